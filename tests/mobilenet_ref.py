"""Test-side restatement of AdelaiDet's MobileNetV2 bottom-up (adet/modeling/backbone/mobilenet.py: the tonylins layout with
FrozenBatchNorm2d, width 1.0, as build_fcos_resnet_fpn_backbone builds it with MODEL.MOBILENET True).  TEST INFRASTRUCTURE: the
product never imports this file.

features.0 = conv 3x3 stride 2 pad 1, 3 -> 32 + FrozenBN (eps 1e-5) + ReLU6; features.1 .. 17 = InvertedResidual blocks of the table
(t, c, n, s) = (1,16,1,1), (6,24,2,2), (6,32,3,2), (6,64,4,2), (6,96,3,1), (6,160,3,2), (6,320,1,1), the stride on the first block of a
group.  A block's `conv` is nn.Sequential: t = 1: [0] depthwise 3x3, [1] BN, ReLU6, [3] 1x1, [4] BN; t = 6: [0] 1x1 expand, [1] BN, ReLU6,
[3] depthwise 3x3, [4] BN, ReLU6, [6] 1x1, [7] BN.  The input is added only when stride == 1 and cin == cout; nothing follows the add.
No trailing 1x1 to 1280.  res2..res5 are the outputs of features 3 / 6 / 13 / 17: 24 / 32 / 96 / 320 channels at strides 4 / 8 / 16 / 32.

Two forms:
  * fp32 or float64 (whatever dtype x has);
  * a bf16 form that rounds where the HIP graph rounds (oracle.bf16.r): the stem output, and per block the expand output (stored
    BEFORE its ReLU6: the depthwise launch clamps on load, which is the same value because 0 and 6 are exact in bf16 and rounding is
    monotonic), the depthwise output and the block output.  Weights of every conv are bf16 values, FrozenBN scale / shift fp32.
"""
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

from oracle import backbone as OB
from oracle import bf16 as OB16

TABLE = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1))
STAGE_AFTER = {3: "res2", 6: "res3", 13: "res4", 17: "res5"}
PREFIX = "backbone.bottom_up.features"


def blocks() -> List[Tuple[int, int, int, int]]:
    """(cin, t, cout, stride) of features.1 .. features.17"""
    out, cin = [], 32
    for t, c, n, s in TABLE:
        for i in range(n):
            out.append((cin, t, c, s if i == 0 else 1))
            cin = c
    return out


# the 12 distinct block shapes of the network
BLOCK_SHAPES = sorted(set(blocks()), key=blocks().index)


def expected_keys() -> Dict[str, Tuple[int, ...]]:
    """every backbone.bottom_up key of the checkpoint with its shape"""
    out = {}

    def bn(p, c):
        for k in ("weight", "bias", "running_mean", "running_var"):
            out[f"{p}.{k}"] = (c,)

    out[f"{PREFIX}.0.0.weight"] = (32, 3, 3, 3)
    bn(f"{PREFIX}.0.1", 32)
    for fi, (cin, t, cout, _) in enumerate(blocks(), start=1):
        q, hid, j = f"{PREFIX}.{fi}.conv", cin * t, 0
        if t != 1:
            out[f"{q}.0.weight"] = (hid, cin, 1, 1)
            bn(f"{q}.1", hid)
            j = 3
        out[f"{q}.{j}.weight"] = (hid, 1, 3, 3)
        bn(f"{q}.{j + 1}", hid)
        out[f"{q}.{j + 3}.weight"] = (cout, hid, 1, 1)
        bn(f"{q}.{j + 4}", cout)
    return out


def block_params(sd, fi: int, t: int):
    """-> (ws, scales, shifts) of expand (None for t = 1), depthwise, project of features.<fi>"""
    q = f"{PREFIX}.{fi}.conv"
    idx = [None, 0, 3] if t == 1 else [0, 3, 6]
    ws = [None if i is None else sd[f"{q}.{i}.weight"] for i in idx]
    ss = [(None, None) if i is None else OB.bn_scale_shift(sd, f"{q}.{i + 1}") for i in idx]
    return ws, [s[0] for s in ss], [s[1] for s in ss]


def _bn(y, scale, shift):
    return y * scale.to(y.dtype).view(1, -1, 1, 1) + shift.to(y.dtype).view(1, -1, 1, 1)


def relu6(v):
    return v.clamp(0.0, 6.0)


def block(x, ws, scales, shifts, stride, hidden: Optional[list] = None):
    """One InvertedResidual block in x's dtype.  hidden: the tensors after each ReLU6 are appended."""
    h = x
    if ws[0] is not None:
        h = relu6(_bn(F.conv2d(x, ws[0].to(x.dtype)), scales[0], shifts[0]))
        if hidden is not None:
            hidden.append(h)
    h = relu6(_bn(F.conv2d(h, ws[1].to(x.dtype), None, stride=stride, padding=1, groups=h.shape[1]), scales[1], shifts[1]))
    if hidden is not None:
        hidden.append(h)
    y = _bn(F.conv2d(h, ws[2].to(x.dtype)), scales[2], shifts[2])
    return y + x if stride == 1 and x.shape[1] == y.shape[1] else y


def stem(x, sd):
    sc, sh = OB.bn_scale_shift(sd, f"{PREFIX}.0.1")
    return relu6(_bn(F.conv2d(x, sd[f"{PREFIX}.0.0.weight"].to(x.dtype), None, stride=2, padding=1), sc, sh))


def mobilenet(x, sd, hidden: Optional[list] = None, inputs: Optional[list] = None) -> Dict[str, torch.Tensor]:
    """{res2..res5}.  hidden: per block the list of its post-ReLU6 tensors; inputs: every block's input."""
    x = stem(x, sd)
    outs = {}
    for fi, (cin, t, cout, stride) in enumerate(blocks(), start=1):
        hb = [] if hidden is not None else None
        if inputs is not None:
            inputs.append(x)
        x = block(x, *block_params(sd, fi, t), stride, hb)
        if hidden is not None:
            hidden.append(hb)
        if fi in STAGE_AFTER:
            outs[STAGE_AFTER[fi]] = x
    return outs


def mobilenet_backbone_fpn(x, sd):
    """images (B,3,H,W) normalised / padded -> [p3..p7] through oracle.backbone.fpn."""
    sdd = {k: v.to(x.dtype) for k, v in sd.items()}
    f = OB.fpn(mobilenet(x, sdd), sdd)
    return [f[k] for k in ("p3", "p4", "p5", "p6", "p7")]


# ---- bf16 form: rounds where the HIP graph rounds ---------------------------------------------------------------------------------
def block_bf16(x_bf, ws, scales, shifts, stride, expand_the_padding: bool = False):
    """One block as the HIP graph computes it.  expand_the_padding: the WRONG variant a fused kernel produces when it runs the expand on
    the zero halo of its input tile -- the depthwise conv then sees relu6(shift) instead of zero outside the image."""
    r = OB16.r
    h1 = x_bf
    if ws[0] is not None:
        xin = F.pad(x_bf, (1, 1, 1, 1)) if expand_the_padding else x_bf
        h1 = r(OB16.fma(F.conv2d(xin, r(ws[0])), scales[0].view(1, -1, 1, 1), shifts[0].view(1, -1, 1, 1)))  # stored before its ReLU6
    a1 = relu6(h1)
    pad = 0 if (expand_the_padding and ws[0] is not None) else 1
    acc = F.conv2d(a1, r(ws[1]), None, stride=stride, padding=pad, groups=a1.shape[1])
    h2 = r(relu6(OB16.fma(acc, scales[1].view(1, -1, 1, 1), shifts[1].view(1, -1, 1, 1))))
    v = OB16.fma(F.conv2d(h2, r(ws[2])), scales[2].view(1, -1, 1, 1), shifts[2].view(1, -1, 1, 1))
    if stride == 1 and x_bf.shape[1] == v.shape[1]:
        v = v + x_bf
    return r(v)


def stem_bf16(x_bf, sd):
    sc, sh = OB.bn_scale_shift(sd, f"{PREFIX}.0.1")
    acc = F.conv2d(x_bf, OB16.r(sd[f"{PREFIX}.0.0.weight"]), None, stride=2, padding=1)
    return OB16.r(relu6(OB16.fma(acc, sc.view(1, -1, 1, 1), sh.view(1, -1, 1, 1))))


def mobilenet_bf16(x_bf, sd, inputs: Optional[list] = None) -> Dict[str, torch.Tensor]:
    x = stem_bf16(x_bf, sd)
    outs = {}
    for fi, (cin, t, cout, stride) in enumerate(blocks(), start=1):
        if inputs is not None:
            inputs.append(x)
        x = block_bf16(x, *block_params(sd, fi, t), stride)
        if fi in STAGE_AFTER:
            outs[STAGE_AFTER[fi]] = x
    return outs


def mobilenet_backbone_fpn_bf16(x_bf, sd):
    f = OB16.fpn(mobilenet_bf16(x_bf, sd), sd)
    return [f[k] for k in ("p3", "p4", "p5", "p6", "p7")]
