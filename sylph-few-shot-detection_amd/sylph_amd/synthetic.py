"""Seeded synthetic weights in the reference's checkpoint key layout and synthetic query / support
inputs: what bench.py, the smoke test and the parity tests feed to BOTH the HIP path and the CPU oracle.
Pure data generation: no model arithmetic, no dependency on oracle/.

Key layout (state_dict of sylph MetaOneStageDetector, captured from the reference modules):
  backbone.bottom_up.stem.conv1.{weight,norm.*}, backbone.bottom_up.res{2..5}.{i}.{shortcut,conv1,
  conv2,conv3}.{weight,norm.{weight,bias,running_mean,running_var}}, backbone.fpn_lateral{3,4,5}.*,
  backbone.fpn_output{3,4,5}.*, backbone.top_block.p{6,7}.*,
  proposal_generator.fcos_head.{cls_tower,bbox_tower}.{0,3,6,9}.{weight,bias} (+GN 1,4,7,10),
  ...cls_logits/bbox_pred/ctrness/iou_overlap/scales.{l}.scale  (sylph/modeling/meta_fcos/fcos.py:382-461)
  code_generator.code_generator_head.{support_set_shared_tower.{0,3}(+GN 1,4), post_norm,
  support_set_cls_conv.0, support_set_cls_bias.0, bias_scale.scale, conv_scale.scale, init_norm.{l}}
  (sylph/modeling/code_generator/code_generator.py:277-439)
"""
import math
from typing import Dict, List, Tuple

import torch

STAGE_BLOCKS = {18: (2, 2, 2, 2), 34: (3, 4, 6, 3), 50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}  # detectron2 ResNet depths
BASIC_DEPTHS = (18, 34)  # detectron2 BasicBlock: two 3x3 convs per block, stage widths 64 << s (RES2_OUT_CHANNELS 64)


def _conv(g, cout, cin, k, std=None):
    fan_in = cin * k * k
    std = math.sqrt(2.0 / fan_in) if std is None else std
    return torch.randn(cout, cin, k, k, generator=g) * std


def _bn(g, sd, prefix, c):
    sd[prefix + ".weight"] = torch.rand(c, generator=g) + 0.5
    sd[prefix + ".bias"] = torch.randn(c, generator=g) * 0.1
    sd[prefix + ".running_mean"] = torch.randn(c, generator=g) * 0.1
    sd[prefix + ".running_var"] = torch.rand(c, generator=g) + 0.5


def _gn(g, sd, prefix, c):
    sd[prefix + ".weight"] = 1.0 + 0.1 * torch.randn(c, generator=g)
    sd[prefix + ".bias"] = 0.1 * torch.randn(c, generator=g)


def backbone_state_dict(seed: int = 0, depth: int = 50, num_groups: int = 1, width_per_group: int = 64) -> Dict[str, torch.Tensor]:
    """num_groups / width_per_group (MODEL.RESNETS.*): a ResNeXt backbone (detectron2 build_resnet_backbone) with bottleneck width
    num_groups * width_per_group << stage and conv2 weights (mid, mid / num_groups, 3, 3).  Its conv1 / conv2 / conv3 tensors come
    from a generator of their own, so the default (1 x 64) dict is unchanged.
    depth 18 / 34: BasicBlock backbones -- per block conv1 (cout, cin, 3, 3), conv2 (cout, cout, 3, 3, scaled x 0.25 as conv3 is), a
    shortcut only where the width changes (res3.0, res4.0, res5.0), no conv3; FPN laterals read 128 / 256 / 512 channels."""
    if depth in BASIC_DEPTHS:
        assert (num_groups, width_per_group) == (1, 64), "BasicBlock backbones have no groups"
        return _basic_backbone_state_dict(seed, depth)
    g = torch.Generator().manual_seed(seed)
    grouped = (num_groups, width_per_group) != (1, 64)
    gx = torch.Generator().manual_seed(seed + 7919) if grouped else g
    sd = {}
    p = "backbone.bottom_up"
    # inputs are O(100) (0..255 minus mean): scale the stem so activations are O(1)
    sd[f"{p}.stem.conv1.weight"] = _conv(g, 64, 3, 7) / 64.0
    _bn(g, sd, f"{p}.stem.conv1.norm", 64)
    cin = 64
    for si, nb in enumerate(STAGE_BLOCKS[depth]):
        stage = si + 2
        mid, cout = (num_groups * width_per_group) << si, 256 * 2 ** si
        for bi in range(nb):
            q = f"{p}.res{stage}.{bi}"
            if bi == 0:
                sd[f"{q}.shortcut.weight"] = _conv(g, cout, cin, 1)
                _bn(g, sd, f"{q}.shortcut.norm", cout)
            sd[f"{q}.conv1.weight"] = _conv(gx, mid, cin, 1)
            _bn(gx, sd, f"{q}.conv1.norm", mid)
            sd[f"{q}.conv2.weight"] = _conv(gx, mid, mid // num_groups, 3)
            _bn(gx, sd, f"{q}.conv2.norm", mid)
            # keep the residual branch small so activations stay O(1) through 16-33 blocks
            sd[f"{q}.conv3.weight"] = _conv(gx, cout, mid, 1) * 0.25
            _bn(gx, sd, f"{q}.conv3.norm", cout)
            cin = cout
    for stage, c in ((3, 512), (4, 1024), (5, 2048)):
        sd[f"backbone.fpn_lateral{stage}.weight"] = _conv(g, 256, c, 1, std=math.sqrt(1.0 / c))
        sd[f"backbone.fpn_lateral{stage}.bias"] = torch.randn(256, generator=g) * 0.1
        sd[f"backbone.fpn_output{stage}.weight"] = _conv(g, 256, 256, 3, std=math.sqrt(1.0 / 2304))
        sd[f"backbone.fpn_output{stage}.bias"] = torch.randn(256, generator=g) * 0.1
    for n in ("p6", "p7"):
        sd[f"backbone.top_block.{n}.weight"] = _conv(g, 256, 256, 3, std=math.sqrt(1.0 / 2304))
        sd[f"backbone.top_block.{n}.bias"] = torch.randn(256, generator=g) * 0.1
    return sd


def _basic_backbone_state_dict(seed: int, depth: int) -> Dict[str, torch.Tensor]:
    g = torch.Generator().manual_seed(seed)
    sd = {}
    p = "backbone.bottom_up"
    sd[f"{p}.stem.conv1.weight"] = _conv(g, 64, 3, 7) / 64.0
    _bn(g, sd, f"{p}.stem.conv1.norm", 64)
    cin = 64
    for si, nb in enumerate(STAGE_BLOCKS[depth]):
        cout = 64 << si
        for bi in range(nb):
            q = f"{p}.res{si + 2}.{bi}"
            if cin != cout:
                sd[f"{q}.shortcut.weight"] = _conv(g, cout, cin, 1)
                _bn(g, sd, f"{q}.shortcut.norm", cout)
            sd[f"{q}.conv1.weight"] = _conv(g, cout, cin, 3)
            _bn(g, sd, f"{q}.conv1.norm", cout)
            # keep the residual branch small so activations stay O(1) through the blocks
            sd[f"{q}.conv2.weight"] = _conv(g, cout, cout, 3) * 0.25
            _bn(g, sd, f"{q}.conv2.norm", cout)
            cin = cout
    for stage, c in ((3, 128), (4, 256), (5, 512)):
        sd[f"backbone.fpn_lateral{stage}.weight"] = _conv(g, 256, c, 1, std=math.sqrt(1.0 / c))
        sd[f"backbone.fpn_lateral{stage}.bias"] = torch.randn(256, generator=g) * 0.1
        sd[f"backbone.fpn_output{stage}.weight"] = _conv(g, 256, 256, 3, std=math.sqrt(1.0 / 2304))
        sd[f"backbone.fpn_output{stage}.bias"] = torch.randn(256, generator=g) * 0.1
    for n in ("p6", "p7"):
        sd[f"backbone.top_block.{n}.weight"] = _conv(g, 256, 256, 3, std=math.sqrt(1.0 / 2304))
        sd[f"backbone.top_block.{n}.bias"] = torch.randn(256, generator=g) * 0.1
    return sd


MOBILENET_V2_TABLE = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1))  # (t, c, n, s)


def mobilenet_v2_blocks() -> List[Tuple[int, int, int, int]]:
    """(cin, t, cout, stride) of features.1 .. features.17 (width 1.0; the stride sits on the first block of a group)."""
    out, cin = [], 32
    for t, c, n, s in MOBILENET_V2_TABLE:
        for i in range(n):
            out.append((cin, t, c, s if i == 0 else 1))
            cin = c
    return out


def mobilenet_backbone_state_dict(seed: int = 0) -> Dict[str, torch.Tensor]:
    """AdelaiDet's MobileNetV2 bottom-up (adet/modeling/backbone/mobilenet.py, the tonylins layout with FrozenBatchNorm2d) + the FPN on
    res3 / res4 / res5 = features 6 / 13 / 17 (32 / 96 / 320 channels).  Keys: backbone.bottom_up.features.0.{0.weight, 1.*} (conv 3x3 s2
    3 -> 32, BN), features.{1..17}.conv.{i}: t = 1: 0 depthwise, 1 BN, 3 project, 4 BN; t = 6: 0 expand, 1 BN, 3 depthwise, 4 BN, 6 project,
    7 BN.  A generator of its own: no key of the ResNet dicts changes.
    The gains put real work on both clamps of every ReLU6: pre-activations with a standard deviation of 3 to 6 around +1 (a few per
    cent above 6, a third below 0), projections small enough that 17 blocks with up to three residual adds in a row stay O(1)."""
    g = torch.Generator().manual_seed(seed + 104729)
    sd = {}
    p = "backbone.bottom_up.features"

    def bn(prefix, c, bias0):
        sd[prefix + ".weight"] = torch.rand(c, generator=g) * 0.5 + 0.75
        sd[prefix + ".bias"] = torch.randn(c, generator=g) * 0.3 + bias0
        sd[prefix + ".running_mean"] = torch.randn(c, generator=g) * 0.1
        sd[prefix + ".running_var"] = torch.rand(c, generator=g) * 0.5 + 0.75

    # inputs are O(100) (0..255 minus the mean, rms ~75): pre-activation std ~3
    sd[f"{p}.0.0.weight"] = torch.randn(32, 3, 3, 3, generator=g) * (3.0 / (75.0 * math.sqrt(27.0)))
    bn(f"{p}.0.1", 32, 1.0)
    for fi, (cin, t, cout, stride) in enumerate(mobilenet_v2_blocks(), start=1):
        q, hid, j = f"{p}.{fi}.conv", cin * t, 0
        if t != 1:
            sd[f"{q}.0.weight"] = torch.randn(hid, cin, 1, 1, generator=g) * (4.0 / math.sqrt(cin))  # block inputs have rms 0.6 .. 1.5
            bn(f"{q}.1", hid, 1.0)
            j = 3
        sd[f"{q}.{j}.weight"] = torch.randn(hid, 1, 3, 3, generator=g) * (1.2 / 3.0)  # inputs in [0, 6], rms ~2.3
        bn(f"{q}.{j + 1}", hid, 0.5)
        sd[f"{q}.{j + 3}.weight"] = torch.randn(cout, hid, 1, 1, generator=g) * (0.35 / math.sqrt(hid))
        bn(f"{q}.{j + 4}", cout, 0.0)
    for stage, c in ((3, 32), (4, 96), (5, 320)):
        sd[f"backbone.fpn_lateral{stage}.weight"] = _conv(g, 256, c, 1, std=math.sqrt(1.0 / c))
        sd[f"backbone.fpn_lateral{stage}.bias"] = torch.randn(256, generator=g) * 0.1
        sd[f"backbone.fpn_output{stage}.weight"] = _conv(g, 256, 256, 3, std=math.sqrt(1.0 / 2304))
        sd[f"backbone.fpn_output{stage}.bias"] = torch.randn(256, generator=g) * 0.1
    for n in ("p6", "p7"):
        sd[f"backbone.top_block.{n}.weight"] = _conv(g, 256, 256, 3, std=math.sqrt(1.0 / 2304))
        sd[f"backbone.top_block.{n}.bias"] = torch.randn(256, generator=g) * 0.1
    return sd


def head_state_dict(seed: int = 1, num_classes: int = 60, c: int = 256, num_convs: int = 4,
                    levels: int = 5, num_share_convs: int = 0, norm: str = "GN", num_cls_convs: int = None,
                    num_box_convs: int = None, deformable: bool = False) -> Dict[str, torch.Tensor]:
    """MetaFCOSHead weights under the reference's keys.  norm "GN": a tower is nn.Sequential(conv, GroupNorm, ReLU) x n (indices 3i,
    3i + 1); norm "none": (conv, ReLU) x n (index 2i) -- fcos.py:72-122.  num_share_convs: the shared tower in front of both.
    deformable (MODEL.FCOS.USE_DEFORMABLE): the last conv of the cls and of the bbox tower is adet's DFConv2d, keys
    {k}.offset.weight [27,256,3,3], {k}.offset.bias, {k}.conv.weight, {k}.conv.bias instead of {k}.weight / {k}.bias."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    p = "proposal_generator.fcos_head"
    step = 3 if norm == "GN" else 2
    for t, n in (("cls_tower", num_convs if num_cls_convs is None else num_cls_convs),
                 ("bbox_tower", num_convs if num_box_convs is None else num_box_convs)):  # MODEL.FCOS.NUM_CLS_CONVS / NUM_BOX_CONVS
        for i in range(n):
            sd[f"{p}.{t}.{step * i}.weight"] = _conv(g, c, c, 3, std=math.sqrt(2.0 / (9 * c)))
            sd[f"{p}.{t}.{step * i}.bias"] = torch.randn(c, generator=g) * 0.1
            if norm == "GN":
                _gn(g, sd, f"{p}.{t}.{step * i + 1}", c)
    g2 = torch.Generator().manual_seed(seed * 7 + 3)  # a separate stream: the keys above stay bit-stable when a shared tower is added
    for i in range(num_share_convs):
        sd[f"{p}.share_tower.{step * i}.weight"] = _conv(g2, c, c, 3, std=math.sqrt(2.0 / (9 * c)))
        sd[f"{p}.share_tower.{step * i}.bias"] = torch.randn(c, generator=g2) * 0.1
        if norm == "GN":
            _gn(g2, sd, f"{p}.share_tower.{step * i + 1}", c)
    if deformable:
        # a separate stream again: every other key stays bit-stable.  Offset rows are scaled so that on a GroupNorm + ReLU input (E x^2 ~ 0.5)
        # the offsets have a std of ~2 px (fractional, many crossing a level border, some far off the map) and the mask logits ~1.5
        # (sigmoid not saturated); zero offsets would hide every sampling bug.
        g3 = torch.Generator().manual_seed(seed * 11 + 5)
        fan = 9 * c * 0.5
        for t, n in (("cls_tower", num_convs if num_cls_convs is None else num_cls_convs),
                     ("bbox_tower", num_convs if num_box_convs is None else num_box_convs)):
            if n == 0:
                continue
            k = step * (n - 1)
            del sd[f"{p}.{t}.{k}.weight"], sd[f"{p}.{t}.{k}.bias"]
            row_std = torch.cat([torch.full((18,), 2.0), torch.full((9,), 1.5)]) / math.sqrt(fan)
            sd[f"{p}.{t}.{k}.offset.weight"] = torch.randn(27, c, 3, 3, generator=g3) * row_std.view(27, 1, 1, 1)
            sd[f"{p}.{t}.{k}.offset.bias"] = torch.cat([torch.randn(18, generator=g3), 0.5 * torch.randn(9, generator=g3)])
            sd[f"{p}.{t}.{k}.conv.weight"] = _conv(g3, c, c, 3, std=math.sqrt(2.0 / (9 * c)))
            sd[f"{p}.{t}.{k}.conv.bias"] = torch.randn(c, generator=g3) * 0.1
    sd[f"{p}.cls_logits.weight"] = _conv(g, num_classes, c, 1, std=0.01)
    sd[f"{p}.cls_logits.bias"] = torch.full((num_classes,), -math.log(99.0))
    sd[f"{p}.bbox_pred.weight"] = _conv(g, 4, c, 3, std=0.02)
    sd[f"{p}.bbox_pred.bias"] = torch.rand(4, generator=g) * 2.0 + 1.0
    sd[f"{p}.ctrness.weight"] = _conv(g, 1, c, 3, std=0.02)
    sd[f"{p}.ctrness.bias"] = torch.randn(1, generator=g) * 0.1
    sd[f"{p}.iou_overlap.weight"] = _conv(g, 1, c, 3, std=0.02)
    sd[f"{p}.iou_overlap.bias"] = torch.randn(1, generator=g) * 0.1
    for l in range(levels):
        sd[f"{p}.scales.{l}.scale"] = torch.tensor([1.0 + 0.1 * l])
    return sd


def codegen_state_dict(seed: int = 2, c: int = 256, out_c: int = 256, tower_layers: int = 2,
                       levels: int = 5, weight_scale_layers: bool = False, tower_spec=None) -> Dict[str, torch.Tensor]:
    g = torch.Generator().manual_seed(seed)
    sd = {}
    p = "code_generator.code_generator_head"
    for l in range(levels):
        _gn(g, sd, f"{p}.init_norm.{l}", c)
    # tower_spec: CODE_GENERATOR.TOWER_LAYERS as [[norm, act], ...] (default: tower_layers x ["GN", "ReLU"]); the nn.Sequential index
    # advances by one per module that exists (conv, [norm], [act]) -- code_generator.py:648-688
    spec = tower_spec if tower_spec is not None else [["GN", "ReLU"]] * tower_layers
    idx = 0
    for norm, act in spec:
        sd[f"{p}.support_set_shared_tower.{idx}.weight"] = _conv(g, c, c, 3, std=math.sqrt(2.0 / (9 * c)))
        sd[f"{p}.support_set_shared_tower.{idx}.bias"] = torch.randn(c, generator=g) * 0.1
        idx += 1
        if norm == "GN":
            _gn(g, sd, f"{p}.support_set_shared_tower.{idx}", c)
            idx += 1
        if act in ("ReLU", "Tanh"):
            idx += 1
    _gn(g, sd, f"{p}.post_norm", out_c)
    sd[f"{p}.support_set_cls_conv.0.weight"] = _conv(g, out_c, c, 3, std=math.sqrt(1.0 / (9 * c)))
    sd[f"{p}.support_set_cls_conv.0.bias"] = torch.randn(out_c, generator=g) * 0.1
    sd[f"{p}.support_set_cls_bias.0.weight"] = _conv(g, 1, c, 3, std=math.sqrt(1.0 / (9 * c)))
    sd[f"{p}.support_set_cls_bias.0.bias"] = torch.randn(1, generator=g) * 0.1
    sd[f"{p}.bias_scale.scale"] = torch.tensor([0.9])
    sd[f"{p}.conv_scale.scale"] = torch.tensor([1.3])
    if weight_scale_layers:  # CODE_GENERATOR.WEIGHT_LAYER / SCALE_LAYER heads (own generator: the weights above stay what they were)
        g2 = torch.Generator().manual_seed(seed + 1000)
        for head, bias0 in (("support_set_cls_weight", 0.0), ("support_set_cls_scale", 1.0)):
            sd[f"{p}.{head}.0.weight"] = _conv(g2, 1, c, 3, std=math.sqrt(4.0 / (9 * c)))
            sd[f"{p}.{head}.0.bias"] = torch.randn(1, generator=g2) * 0.1 + bias0
    return sd


def synthetic_state_dict(seed: int = 0, depth: int = 50, num_classes: int = 60, mobilenet: bool = False) -> Dict[str, torch.Tensor]:
    """mobilenet (MODEL.MOBILENET): the MobileNetV2 bottom-up instead of the ResNet of `depth`; head and code generator are the same."""
    sd = {"pixel_mean": torch.tensor([103.530, 116.280, 123.675]).view(3, 1, 1),
          "pixel_std": torch.tensor([1.0, 1.0, 1.0]).view(3, 1, 1)}
    sd.update(mobilenet_backbone_state_dict(seed) if mobilenet else backbone_state_dict(seed, depth))
    sd.update(head_state_dict(seed + 1, num_classes))
    sd.update(codegen_state_dict(seed + 2))
    return sd


def synthetic_images(n: int, h: int, w: int, seed: int = 1) -> List[torch.Tensor]:
    """uint8-valued fp32 BGR images (3,H,W) in [0,255]."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (3, h, w), generator=g).float() for _ in range(n)]


def synthetic_boxes(n: int, h: int, w: int, seed: int = 2) -> torch.Tensor:
    """One XYXY box per support image: x0,y0 ~ U(0, 0.5*W/H); w,h ~ U(32, 0.5*min)."""
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(n, generator=g) * 0.5 * w
    y0 = torch.rand(n, generator=g) * 0.5 * h
    m = 0.5 * min(h, w)
    lo = min(32.0, 0.5 * m)
    bw = lo + torch.rand(n, generator=g) * (m - lo)
    bh = lo + torch.rand(n, generator=g) * (m - lo)
    return torch.stack([x0, y0, x0 + bw, y0 + bh], dim=1)


def synthetic_codes(n: int, c: int = 256, seed: int = 3, scale: float = 1.0) -> Dict[str, torch.Tensor]:
    """Normalised-looking class codes: unit-L2 rows x scale, bias at the focal prior."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, c, 1, 1, generator=g)
    w = w / w.flatten(1).norm(dim=1).view(n, 1, 1, 1) * scale
    return {"cls_conv": w, "cls_bias": torch.full((n,), -math.log(99.0)) + 0.1 * torch.randn(n, generator=g)}


def roi_encoder_state_dict(seed: int = 4, c: int = 256, inter: int = 64, fc_dim: int = 256, head_fc: int = 512,
                           layers: int = 2, tok_convs: int = 2, tok_fcs: int = 2) -> Dict[str, torch.Tensor]:
    """Seeded weights in the key layout of the reference ROIEncoder module
    (sylph/modeling/code_generator/roi_encoder.py:206-281, utils.py:70-141)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    p = "code_generator"

    def lin(name, o, i, std=None):
        sd[f"{name}.weight"] = torch.randn(o, i, generator=g) * (std if std is not None else math.sqrt(1.0 / i))
        sd[f"{name}.bias"] = torch.randn(o, generator=g) * 0.1

    def gn(name, ch):
        sd[f"{name}.weight"] = 1.0 + 0.1 * torch.randn(ch, generator=g)
        sd[f"{name}.bias"] = 0.1 * torch.randn(ch, generator=g)

    sd[f"{p}.box_pooler.conv.0.weight"] = _conv(g, c, c, 3, std=math.sqrt(2.0 / (9 * c)))
    sd[f"{p}.box_pooler.conv.0.bias"] = torch.randn(c, generator=g) * 0.1
    gn(f"{p}.box_pooler.conv.1", c)
    cam = f"{p}.box_pooler.context_attention_module"
    for branch, idx in (("local_att", (0, 1, 3, 4)), ("global_att", (1, 2, 4, 5))):
        sd[f"{cam}.{branch}.{idx[0]}.weight"] = _conv(g, inter, c, 1, std=math.sqrt(1.0 / c))
        sd[f"{cam}.{branch}.{idx[0]}.bias"] = torch.randn(inter, generator=g) * 0.1
        gn(f"{cam}.{branch}.{idx[1]}", inter)
        sd[f"{cam}.{branch}.{idx[2]}.weight"] = _conv(g, c, inter, 1, std=math.sqrt(1.0 / inter))
        sd[f"{cam}.{branch}.{idx[2]}.bias"] = torch.randn(c, generator=g) * 0.1
        gn(f"{cam}.{branch}.{idx[3]}", c)
    for k in range(tok_convs):
        sd[f"{p}.tokenizer.conv{k + 1}.weight"] = _conv(g, c, c, 3, std=math.sqrt(2.0 / (9 * c)))
        gn(f"{p}.tokenizer.conv{k + 1}.norm", c)
    din = c * 49
    for k in range(tok_fcs):
        lin(f"{p}.tokenizer.fc{k + 1}", fc_dim, din, std=math.sqrt(2.0 / din))
        din = fc_dim
    for l in range(layers):
        q = f"{p}.transformer_encoder.layers.{l}"
        sd[f"{q}.self_attn.in_proj_weight"] = torch.randn(3 * fc_dim, fc_dim, generator=g) * math.sqrt(1.0 / fc_dim)
        sd[f"{q}.self_attn.in_proj_bias"] = torch.randn(3 * fc_dim, generator=g) * 0.1
        lin(f"{q}.self_attn.out_proj", fc_dim, fc_dim)
        lin(f"{q}.linear1", 4 * fc_dim, fc_dim, std=math.sqrt(2.0 / fc_dim))
        lin(f"{q}.linear2", fc_dim, 4 * fc_dim)
        gn(f"{q}.norm1", fc_dim)
        gn(f"{q}.norm2", fc_dim)
    lin(f"{p}.weight_head.fc1", head_fc, fc_dim, std=math.sqrt(2.0 / fc_dim))
    lin(f"{p}.weight_head.fc2", c, head_fc)
    lin(f"{p}.bias_head.fc1", head_fc, fc_dim, std=math.sqrt(2.0 / fc_dim))
    lin(f"{p}.bias_head.fc2", 1, head_fc)
    sd["proposal_generator.fcos_head.cond_cls_logits.scales.0.scale"] = torch.tensor([0.8])
    return sd
