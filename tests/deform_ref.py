"""Test-side restatement of the modulated deformable 3x3 conv (DCNv2) of a deformable FCOS tower (MODEL.FCOS.USE_DEFORMABLE).
TEST INFRASTRUCTURE: the product never imports this file.

adet's DFConv2d(256, 256, 3, stride 1, padding 1, bias=True) with its defaults (with_modulated_dcn, deformable_groups 1):
  om = conv3x3(x, offset.weight, offset.bias, pad 1)          channels 0..17 offsets, 18..26 mask logits
  tap j = 3 ky + kx:  dy = om[2j], dx = om[2j + 1], mask = sigmoid(om[18 + j])
  the tap samples x at (y - 1 + ky + dy, x - 1 + kx + dx): 0 unless -1 < py < H and -1 < px < W, otherwise the bilinear blend of
  the neighbours floor(p) + {0, 1}, each neighbour outside the map contributing 0 (detectron2 dmcn_im2col_bilinear)
  out[y, x, :] = conv.bias + sum_j W[:, :, ky, kx] . (mask_j * sample_j)

Three forms:
  * deform_conv_loop: explicit float64 loops written from the statement above;
  * deform_conv_grid_sample: F.grid_sample(bilinear, zeros, align_corners=True) on normalised coordinates;
  * deform_conv_bf16: rounds where csrc/conv_deform.hip rounds -- bf16 input, fp32 offsets, the fp32 blend
    (((v00 w00 + v01 w01) + v10 w10) + v11 w11) * mask, the A operand rounded to bf16 -- then an fp32-exact product sum.
deform_fcos_head mirrors oracle.head.fcos_head with the deformable last tower layer, for every tower variant the head builder accepts:
a shared tower in front (never deformable), towers of depth 0 (no layer at all) and 1 (the deformable layer reads the tower input),
unequal depths, MODEL.FCOS.NORM "none", 3x3 class codes, and maps under 2 x 2 (deform_conv_any: the loop form there).
"""
import math
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

from oracle.head import GN_EPS, GN_GROUPS, HEAD_PREFIX, cond_conv_basic, cond_conv_block
from oracle.head import tower as plain_tower


def offset_conv(x: torch.Tensor, ow: torch.Tensor, ob: torch.Tensor) -> torch.Tensor:
    return F.conv2d(x, ow, ob, padding=1)


def deform_conv_loop(x: torch.Tensor, om: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor]) -> torch.Tensor:
    """(a) explicit loops, float64.  x (B, C, H, W), om (B, 27, H, W), w (Co, C, 3, 3) -> (B, Co, H, W)."""
    x, om, w = x.double(), om.double(), w.double()
    B, C, H, W = x.shape
    out = torch.zeros(B, w.shape[0], H, W, dtype=torch.float64)
    for n in range(B):
        for y in range(H):
            for xx in range(W):
                col = torch.zeros(C, 9, dtype=torch.float64)
                for ky in range(3):
                    for kx in range(3):
                        j = 3 * ky + kx
                        py = (y - 1 + ky) + float(om[n, 2 * j, y, xx])
                        px = (xx - 1 + kx) + float(om[n, 2 * j + 1, y, xx])
                        m = 1.0 / (1.0 + math.exp(-float(om[n, 18 + j, y, xx])))
                        if not (-1 < py < H and -1 < px < W):
                            continue
                        y0, x0 = math.floor(py), math.floor(px)
                        lh, lw = py - y0, px - x0
                        v = torch.zeros(C, dtype=torch.float64)
                        for yy, xq, wgt in ((y0, x0, (1 - lh) * (1 - lw)), (y0, x0 + 1, (1 - lh) * lw),
                                            (y0 + 1, x0, lh * (1 - lw)), (y0 + 1, x0 + 1, lh * lw)):
                            if 0 <= yy < H and 0 <= xq < W:
                                v = v + wgt * x[n, :, yy, xq]
                        col[:, j] = m * v
                out[n, :, y, xx] = torch.einsum("ocj,cj->o", w.reshape(w.shape[0], C, 9), col)
    if b is not None:
        out = out + b.double().view(1, -1, 1, 1)
    return out


def deform_conv_grid_sample(x: torch.Tensor, om: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor]) -> torch.Tensor:
    """(b) F.grid_sample on normalised coordinates, float64 (maps of at least 2 x 2)."""
    x, om, w = x.double(), om.double(), w.double()
    B, C, H, W = x.shape
    ys = torch.arange(H, dtype=torch.float64).view(1, H, 1)
    xs = torch.arange(W, dtype=torch.float64).view(1, 1, W)
    cols = []
    for j in range(9):
        ky, kx = divmod(j, 3)
        py = ys - 1 + ky + om[:, 2 * j]
        px = xs - 1 + kx + om[:, 2 * j + 1]
        grid = torch.stack([px / (W - 1) * 2 - 1, py / (H - 1) * 2 - 1], dim=-1)
        s = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
        cols.append(s * torch.sigmoid(om[:, 18 + j]).unsqueeze(1))
    col = torch.stack(cols, dim=2)  # B, C, 9, H, W
    out = torch.einsum("ocj,bcjhw->bohw", w.reshape(w.shape[0], C, 9), col)
    if b is not None:
        out = out + b.double().view(1, -1, 1, 1)
    return out


def _bf16(t: torch.Tensor) -> torch.Tensor:
    return t.float().bfloat16().float()


def sample_fp32(x: torch.Tensor, om: torch.Tensor, round_bf16: bool) -> torch.Tensor:
    """The kernel's A operand: (B, 9, C, H, W) float32, blended in fp32 in the kernel's fixed order, optionally rounded to bf16."""
    x, om = x.float(), om.float()
    B, C, H, W = x.shape
    dev = x.device
    yi = torch.arange(H, device=dev, dtype=torch.int32).view(1, H, 1)
    xi = torch.arange(W, device=dev, dtype=torch.int32).view(1, 1, W)
    flat = x.reshape(B, C, H * W)
    out = torch.empty(B, 9, C, H, W, dtype=torch.float32, device=dev)
    for j in range(9):
        ky, kx = divmod(j, 3)
        py = (yi - 1 + ky).float() + om[:, 2 * j]
        px = (xi - 1 + kx).float() + om[:, 2 * j + 1]
        mask = 1.0 / (1.0 + torch.exp(-om[:, 18 + j]))
        inside = (py > -1) & (px > -1) & (py < H) & (px < W)
        fy, fx = torch.floor(py), torch.floor(px)
        lh, lw = py - fy, px - fx
        hh, hw = 1.0 - lh, 1.0 - lw
        fy = torch.where(inside, fy, torch.zeros_like(fy)).long()
        fx = torch.where(inside, fx, torch.zeros_like(fx)).long()
        acc = None
        for dyi, dxi, wgt in ((0, 0, hh * hw), (0, 1, hh * lw), (1, 0, lh * hw), (1, 1, lh * lw)):
            yy, xq = fy + dyi, fx + dxi
            ok = inside & (yy >= 0) & (yy < H) & (xq >= 0) & (xq < W)
            idx = (yy.clamp(0, H - 1) * W + xq.clamp(0, W - 1)).view(B, 1, H * W).expand(B, C, H * W)
            v = torch.gather(flat, 2, idx).view(B, C, H, W) * ok.unsqueeze(1).float()
            term = v * torch.where(inside, wgt, torch.zeros_like(wgt)).unsqueeze(1)
            acc = term if acc is None else acc + term
        a = acc * mask.unsqueeze(1)
        out[:, j] = _bf16(a) if round_bf16 else a
    return out


def deform_conv_from_samples(A: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], dtype=torch.float64) -> torch.Tensor:
    B, _, C, H, W = A.shape
    wm = w.to(dtype).reshape(w.shape[0], C, 3, 3).permute(0, 2, 3, 1).reshape(w.shape[0], 9 * C)  # [o][tap][c]
    out = torch.matmul(wm, A.to(dtype).reshape(B, 9 * C, H * W)).view(B, -1, H, W)
    if b is not None:
        out = out + b.to(dtype).view(1, -1, 1, 1)
    return out


def deform_conv_bf16(x_bf: torch.Tensor, om: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """bf16-storage form: x_bf exact bf16 values, om fp32; returns the fp64 conv of the bf16 A operand with bf16 weights (+ fp32 bias)."""
    A = sample_fp32(x_bf, om.float(), round_bf16=True)
    return deform_conv_from_samples(A, _bf16(w), b.float())


def deform_conv_any(x: torch.Tensor, om: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor]) -> torch.Tensor:
    """deform_conv_grid_sample, and deform_conv_loop on maps under 2 x 2 (a 1-row or 1-column map has no normalised coordinate)."""
    if min(x.shape[-2:]) < 2:
        return deform_conv_loop(x, om, w, b)
    return deform_conv_grid_sample(x, om, w, b)


def deform_tower(x: torch.Tensor, sd: Dict[str, torch.Tensor], prefix: str, num_convs: int = 4, norm: str = "GN",
                 deform=deform_conv_any) -> torch.Tensor:
    """oracle.head.tower for layers 0 .. n-2, then the DFConv2d layer (+ GroupNorm) + ReLU.  num_convs 1: the deformable layer reads the
    tower input itself; num_convs 0: no tower (fcos.py:72-122 builds an empty nn.Sequential) and no deformable layer."""
    if num_convs == 0:
        return x
    step = 2 if norm in ("none", "", None) else 3
    x = plain_tower(x, sd, prefix, num_convs - 1, norm)
    k = step * (num_convs - 1)
    om = offset_conv(x.double(), sd[f"{prefix}.{k}.offset.weight"].double(), sd[f"{prefix}.{k}.offset.bias"].double())
    y = deform(x, om, sd[f"{prefix}.{k}.conv.weight"], sd[f"{prefix}.{k}.conv.bias"]).to(x.dtype)
    if step == 3:
        y = F.group_norm(y, GN_GROUPS, sd[f"{prefix}.{k + 1}.weight"].to(y.dtype), sd[f"{prefix}.{k + 1}.bias"].to(y.dtype), eps=GN_EPS)
    return F.relu(y)


def deform_fcos_head(features: List[torch.Tensor], sd: Dict[str, torch.Tensor], class_codes: Dict[str, torch.Tensor],
                     num_cls_convs: int = 4, num_box_convs: int = 4, use_scale: bool = True, use_bias: bool = True,
                     cond_block: bool = False, prefix: str = HEAD_PREFIX, cond_scales: Optional[List[float]] = None,
                     norm: str = "GN", dtype=torch.float64, num_share_convs: int = 0, deformable: bool = True,
                     deform=deform_conv_any):
    """oracle.head.fcos_head (episodic branch, fcos.py:582-667) with MODEL.FCOS.USE_DEFORMABLE towers; computed in `dtype`.
    num_share_convs: the shared tower in front of both towers, never deformable (fcos.py:388-397, 626).  Class codes (N, 256, k, k) run
    with padding k // 2 (fcos.py:499-510).  deformable False: plain towers, i.e. oracle.head.fcos_head in `dtype`.  deform: the form of
    the deformable conv (deform_conv_any, or deform_conv_loop / deform_conv_grid_sample on every level)."""
    sdd = {k: v.to(dtype) for k, v in sd.items()}
    w = class_codes["cls_conv"].to(dtype)
    b = class_codes["cls_bias"].to(dtype) if class_codes.get("cls_bias") is not None else None

    def one_tower(x, name, n):
        if deformable:
            return deform_tower(x, sdd, f"{prefix}.{name}", n, norm, deform)
        return plain_tower(x, sdd, f"{prefix}.{name}", n, norm)

    logits, regs, ctrs, ious = [], [], [], []
    for level, feat in enumerate(features):
        feat = plain_tower(feat.to(dtype), sdd, f"{prefix}.share_tower", num_share_convs, norm)
        cls_t = one_tower(feat, "cls_tower", num_cls_convs)
        box_t = one_tower(feat, "bbox_tower", num_box_convs)
        if cond_block:
            logit = cond_conv_block(cls_t, w, b, scales=cond_scales)
        else:
            logit = cond_conv_basic(cls_t, w, b, padding=w.shape[-1] // 2, use_bias=use_bias)
        reg = F.conv2d(box_t, sdd[f"{prefix}.bbox_pred.weight"], sdd[f"{prefix}.bbox_pred.bias"], padding=1)
        if use_scale:
            reg = reg * sdd[f"{prefix}.scales.{level}.scale"]
        regs.append(F.relu(reg))
        logits.append(logit)
        ctrs.append(F.conv2d(box_t, sdd[f"{prefix}.ctrness.weight"], sdd[f"{prefix}.ctrness.bias"], padding=1))
        ious.append(F.conv2d(box_t, sdd[f"{prefix}.iou_overlap.weight"], sdd[f"{prefix}.iou_overlap.bias"], padding=1))
    return logits, regs, ctrs, ious
