"""Plain torch restatements of what a 3x3 class code (MODEL.META_LEARN.CODE_GENERATOR.CLS_LAYER = [norm, act, 3]) changes.
TEST INFRASTRUCTURE, fp32 torch CPU like oracle/codegen.py and oracle/head.py, whose unchanged pieces (ROI pooler, shared tower,
FCOS towers, prediction convs) are called, not repeated.

Follows (paths relative to the reference):
  * sylph/modeling/code_generator/code_generator.py:509-540,954  support_set_cls_conv: conv3x3 256 -> 256 + bias on the 7x7 ROI map,
    then GlobalAdaptiveAvgPool2d(k_s = 3) = F.adaptive_avg_pool2d(., (3, 3)); bias / shot-weight / class-scale heads stay global
  * sylph/modeling/code_generator/code_generator.py:778-829      compute_code: one weight per shot for all 2 304 values
  * sylph/modeling/code_generator/code_generator.py:832-875      normalize_code on (1, 256, 3, 3), code_process_module, process_bias
  * sylph/modeling/meta_fcos/fcos.py:499-510, head_utils.py:60-81  CondConvBasic(padding = 1): F.conv2d, a cross-correlation
"""
import math
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

from oracle import codegen as CG
from oracle import head as H
from oracle.codegen import CG_PREFIX, GN_EPS
from oracle.roi_align import roi_pooler


def pool_bins(size: int = 7, k: int = 3):
    """adaptive_avg_pool bins of one axis: [floor(i size / k), ceil((i + 1) size / k)) -- on 7 positions [0,3), [2,5), [4,7)."""
    return [((i * size) // k, -((-(i + 1) * size) // k)) for i in range(k)]


def adaptive_pool(x: torch.Tensor, k: int = 3) -> torch.Tensor:
    """F.adaptive_avg_pool2d(x, (k, k)) written out: the mean of each (overlapping) bin."""
    hb, wb = pool_bins(x.shape[-2], k), pool_bins(x.shape[-1], k)
    rows = [torch.stack([x[..., y0:y1, x0:x1].mean(dim=(-2, -1)) for x0, x1 in wb], dim=-1) for y0, y1 in hb]
    return torch.stack(rows, dim=-2)


def code_from_roi_features(roi: torch.Tensor, sd, k: int = 3, n_tower_layers: int = 2, bias_l2_norm: bool = False,
                           has_weight_layer: bool = False, has_scale_layer: bool = False, tower_spec=None,
                           prefix: str = CG_PREFIX) -> Dict[str, torch.Tensor]:
    """roi (S, 256, 7, 7), all S shots of ONE class -> un-normalised cls_conv (1, 256, k, k), cls_bias (1, 1, 1, 1) and, with a
    SCALE_LAYER, cls_weight_norm (1, 1, 1, 1).  oracle.codegen.code_from_roi_features with the class-code head pooled per bin."""
    f = CG.shared_tower(roi, sd, n_tower_layers, prefix, tower_spec)
    conv = lambda name: F.conv2d(f, sd[f"{prefix}.{name}.0.weight"], sd[f"{prefix}.{name}.0.bias"], padding=1)
    S = roi.shape[0]
    code_feat = adaptive_pool(conv("support_set_cls_conv"), k)  # (S, 256, k, k)
    w = torch.full((1, S, 1, 1, 1), 1.0 / S)
    if has_weight_layer:
        w = torch.softmax(conv("support_set_cls_weight").mean(dim=(2, 3)).view(1, S, 1, 1, 1), dim=1)
    out = {"cls_conv": (w * code_feat.unsqueeze(0)).sum(dim=1)}
    bias_feat = conv("support_set_cls_bias")
    if bias_l2_norm:
        shp = bias_feat.size()
        bias_feat = F.normalize(bias_feat.view(shp[0], shp[1], -1), p=2, dim=2).view(shp)
    out["cls_bias"] = (w * bias_feat.mean(dim=(2, 3)).view(1, S, 1, 1, 1)).sum(dim=1)
    if has_scale_layer:
        out["cls_weight_norm"] = (w * conv("support_set_cls_scale").mean(dim=(2, 3)).view(1, S, 1, 1, 1)).sum(dim=1)
    return out


def code_generator(features: List[torch.Tensor], boxes: torch.Tensor, sd, strides=(8, 16, 32, 64, 128), **kw):
    return code_from_roi_features(roi_pooler(features, boxes, strides, out_size=7), sd, **kw)


def normalize_code(cls_conv: torch.Tensor, cls_bias: torch.Tensor, sd, cls_weight_norm: Optional[torch.Tensor] = None,
                   prior_prob: float = 0.01, prefix: str = CG_PREFIX):
    """(1, 256, k, k), bias -> normalised (1, 256, k, k), (1,).  GroupNorm(32, 256): a group is 8 channels x k^2 taps (72 values for
    k = 3), biased variance, eps 1e-5, per-channel affine; F.normalize(p = 2, dim = 1): per TAP over the 256 channels; x cls_weight_norm
    (a scalar per class) if present; x conv_scale.  The bias path does not see k."""
    n, c, kh, kw = cls_conv.shape
    assert n == 1 and c == 256
    g = cls_conv.reshape(32, 8 * kh * kw)
    g = (g - g.mean(dim=1, keepdim=True)) / torch.sqrt(g.var(dim=1, unbiased=False, keepdim=True) + GN_EPS)
    code = g.reshape(1, c, kh, kw) * sd[f"{prefix}.post_norm.weight"].view(1, c, 1, 1) + sd[f"{prefix}.post_norm.bias"].view(1, c, 1, 1)
    code = code / code.pow(2).sum(dim=1, keepdim=True).sqrt().clamp_min(1e-12)
    if cls_weight_norm is not None:
        code = code * cls_weight_norm.reshape(())
    code = code * sd[f"{prefix}.conv_scale.scale"]
    bias = cls_bias.reshape(1)
    if f"{prefix}.bias_scale.scale" in sd:
        bias = bias * sd[f"{prefix}.bias_scale.scale"]
    return code, bias + torch.tensor(CG.bias_prior(prior_prob), dtype=torch.float32)


def format_codes(records: List[Dict]) -> Dict[str, torch.Tensor]:
    """format_class_codes_shared (meta_learn_evaluation.py:71-103): row c = the record whose support_set_target is c."""
    by = {int(r["support_set_target"]): r["class_code"] for r in records}
    return {"cls_conv": torch.cat([by[c]["cls_conv"] for c in range(len(by))]),
            "cls_bias": torch.cat([by[c]["cls_bias"].reshape(-1) for c in range(len(by))])}


def cond_conv(xn: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """CondConvBasic with padding k // 2: zero padding of the NORMALISED tower output, cross-correlation."""
    return F.conv2d(xn, weight, bias, padding=weight.shape[-1] // 2)


def fcos_head(features: List[torch.Tensor], sd, codes: Dict[str, torch.Tensor], prefix: str = H.HEAD_PREFIX):
    """Per-level logits (B, N, h, w) of the head with k x k codes; the bbox branch is oracle.head.fcos_head's."""
    return [cond_conv(H.tower(f, sd, f"{prefix}.cls_tower"), codes["cls_conv"], codes["cls_bias"]) for f in features]


# ---- synthetic inputs (shared by tests/golden/gen_spatial_codes_golden.py and the GPU tests) -----------------------------------------
def spatial_codes(n, seed, scale):
    """n 3x3 codes that look normalised: every tap has L2 norm `scale` over the channels; biases near the focal prior."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, 256, 3, 3, generator=g)
    w = w / w.norm(dim=1, keepdim=True) * scale
    return {"cls_conv": w, "cls_bias": torch.full((n,), -math.log(99.0)) + 0.1 * torch.randn(n, generator=g)}


def one_tap_codes(seed, scale):
    """Nine classes, class t non-zero at tap (t // 3, t % 3) only."""
    g = torch.Generator().manual_seed(seed)
    w = torch.zeros(9, 256, 3, 3)
    for t in range(9):
        v = torch.randn(256, generator=g)
        w[t, :, t // 3, t % 3] = v / v.norm() * scale
    return {"cls_conv": w, "cls_bias": torch.full((9,), -math.log(99.0)) + 0.1 * torch.randn(9, generator=g)}


# ---- the 1x1-code path, pinned bit for bit (tests/golden/gen_parent_1x1_golden.py writes it with the library of the commit before
# ---- cg_code_ksize, tests/test_spatial_codes_gpu.py replays it on the current build) ---------------------------------------------
def outputs_1x1(golden_dir) -> Dict[str, "np.ndarray"]:
    """What a k = 1 engine computes on the g1 / g3 cases, as numpy arrays: bf16 head outputs and detections for 5 and 20 classes,
    raw support codes (bf16 and fp32; plain, WEIGHT_LAYER + SCALE_LAYER, BIAS_L2_NORM; class form and ROI-list form) and their
    normalisation.  Needs a GPU."""
    import os

    import numpy as np
    from sylph_amd import synthetic as Wt
    from sylph_amd.engine import Engine
    from test_hip_parity import _cfg, _feats
    g1 = np.load(os.path.join(golden_dir, "g1_head_decode.npz"))
    g3 = np.load(os.path.join(golden_dir, "g3_codegen.npz"))
    out = {}
    eng = Engine(_cfg(), dtype="bf16")
    eng.load_state_dict(Wt.head_state_dict(seed=1, num_classes=60))
    eng.import_pyramid(_feats(g1), (128, 160), [tuple(int(v) for v in s) for s in g1["image_sizes"]])
    for tag in ("n5_t50", "n20_t50"):
        eng.head(torch.from_numpy(g1[f"{tag}_cls_conv"]), torch.from_numpy(g1[f"{tag}_cls_bias"]))
        for name, levels in zip(("logits", "reg", "ctr", "iou"), eng.export_head()):
            for l, t in enumerate(levels):
                out[f"head_{tag}_{name}{l}"] = t.cpu().numpy()
        for i, d in enumerate(eng.decode()):
            for k, v in d.items():
                out[f"det_{tag}_img{i}_{k}"] = v.cpu().numpy()
    eng.close()
    over = {"ws": {"MODEL.META_LEARN.CODE_GENERATOR.WEIGHT_LAYER": ["", "", 1], "MODEL.META_LEARN.CODE_GENERATOR.SCALE_LAYER": ["", "", 1]},
            "l2": {"MODEL.META_LEARN.CODE_GENERATOR.BIAS_L2_NORM": True}, "sup": {}}
    for dtype in ("bf16", "f32"):
        for tag in ("sup", "ws", "l2"):
            eng = Engine(_cfg(**over[tag]), dtype=dtype)
            eng.load_state_dict(Wt.codegen_state_dict(seed=2, weight_scale_layers=tag == "ws"))
            rows = []
            for S in (2, 5):
                eng.import_pyramid(_feats(g3, f"s{S}_feat"), (192, 256))
                boxes = torch.from_numpy(g3[f"s{S}_boxes"])
                code = eng.codegen(boxes).clone()
                rows.append(code)
                out[f"code_{dtype}_{tag}_s{S}"] = code.cpu().numpy()
                out[f"rois_{dtype}_{tag}_s{S}"] = eng.codegen_rois(boxes, list(range(S)), [S - 1, 1] if S > 1 else [1]).cpu().numpy()
                if tag == "ws":
                    out[f"wnorm_{dtype}_{tag}_s{S}"] = eng.codegen_weight_norm(2 if S > 1 else 1).cpu().numpy()
            wn = torch.tensor([0.7, 1.3], device=eng.device) if tag == "ws" else None
            out[f"norm_{dtype}_{tag}"] = eng.normalize_codes(torch.stack(rows).contiguous(), wn).cpu().numpy()
            eng.close()
    return out
