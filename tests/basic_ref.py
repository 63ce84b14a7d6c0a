"""Test-side restatement of detectron2's BasicBlock ResNets (build_resnet_backbone with MODEL.RESNETS.DEPTH 18 / 34,
RES2_OUT_CHANNELS 64).  TEST INFRASTRUCTURE: the product never imports this file.

detectron2 BasicBlock(in, out, stride):
  conv1 3x3 pad 1 (stride) + FrozenBN + ReLU -> conv2 3x3 pad 1 + FrozenBN, + shortcut (1x1 stride + FrozenBN when in != out,
  identity otherwise), ReLU.  Stage widths 64 << s (s = 0 for res2), blocks (2, 2, 2, 2) / (3, 4, 6, 3); the first block of res3..res5
  has stride 2; res2.0 keeps 64 channels and has no shortcut.  STRIDE_IN_1X1 does not apply.

Two forms:
  * fp32 or float64 (whatever dtype x has);
  * a bf16 form that rounds where the HIP graph rounds (oracle.bf16.r / conv_epilogue): every conv launch -- conv1, the projection
    shortcut (a launch of its own here, unlike the bottleneck's folded one), conv2 with the residual added in fp32 before the
    ReLU -- stores bf16.
basic_backbone_fpn / basic_backbone_fpn_bf16 drive oracle.backbone.fpn / oracle.bf16.fpn on the restated features.
"""
from typing import Dict

import torch
import torch.nn.functional as F

from oracle import backbone as OB
from oracle import bf16 as OB16

STAGE_BLOCKS = {18: (2, 2, 2, 2), 34: (3, 4, 6, 3)}


def _conv_bn(x, sd, name, stride=1, padding=0, relu=False):
    y = F.conv2d(x, sd[name + ".weight"].to(x.dtype), None, stride=stride, padding=padding)
    sc, sh = OB.bn_scale_shift(sd, name + ".norm")
    y = y * sc.to(x.dtype).view(1, -1, 1, 1) + sh.to(x.dtype).view(1, -1, 1, 1)
    return F.relu(y) if relu else y


def basic_block(x, sd, prefix, stride, has_shortcut):
    out = _conv_bn(x, sd, prefix + ".conv1", stride=stride, padding=1, relu=True)
    out = _conv_bn(out, sd, prefix + ".conv2", padding=1)
    sc = _conv_bn(x, sd, prefix + ".shortcut", stride=stride) if has_shortcut else x
    return F.relu(out + sc)


def resnet(x, sd, depth, prefix="backbone.bottom_up") -> Dict[str, torch.Tensor]:
    """{res2..res5} of the BasicBlock bottom-up (stem as detectron2 BasicStem)."""
    x = _conv_bn(x, sd, prefix + ".stem.conv1", stride=2, padding=3, relu=True)
    x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
    outs = {}
    for si, nb in enumerate(STAGE_BLOCKS[depth]):
        for bi in range(nb):
            first = bi == 0 and si > 0
            x = basic_block(x, sd, f"{prefix}.res{si + 2}.{bi}", 2 if first else 1, first)
        outs[f"res{si + 2}"] = x
    return outs


def basic_backbone_fpn(x, sd, depth):
    """images (B,3,H,W) normalised / padded -> [p3..p7] through oracle.backbone.fpn."""
    sdd = {k: v.to(x.dtype) for k, v in sd.items()}
    f = OB.fpn(resnet(x, sdd, depth), sdd)
    return [f[k] for k in ("p3", "p4", "p5", "p6", "p7")]


# ---- bf16 form: rounds where the HIP graph rounds ---------------------------------------------------------------------------------
def block_params(sd, prefix, has_shortcut):
    """-> (ws, scales, shifts) of conv1, conv2, shortcut (None for an identity block)."""
    names = ["conv1", "conv2"] + (["shortcut"] if has_shortcut else [])
    ws = [sd[f"{prefix}.{n}.weight"] for n in names]
    ss = [OB.bn_scale_shift(sd, f"{prefix}.{n}.norm") for n in names]
    ws, scales, shifts = ws, [s[0] for s in ss], [s[1] for s in ss]
    if not has_shortcut:
        ws, scales, shifts = ws + [None], scales + [None], shifts + [None]
    return ws, scales, shifts


def basic_block_bf16(x_bf, ws, scales, shifts, stride):
    """One block as the HIP graph computes it: t and the projected shortcut stored bf16, the residual added to conv2's fp32 epilogue."""
    _, t = OB16.conv_epilogue(x_bf, ws[0], scales[0], shifts[0], stride=stride, padding=1, relu=True)
    sc = x_bf
    if len(ws) > 2 and ws[2] is not None:
        _, sc = OB16.conv_epilogue(x_bf, ws[2], scales[2], shifts[2], stride=stride)
    _, y = OB16.conv_epilogue(t, ws[1], scales[1], shifts[1], padding=1, relu=True, res_bf=sc)
    return y


def resnet_bf16(x_bf, sd, depth, prefix="backbone.bottom_up") -> Dict[str, torch.Tensor]:
    x = OB16.stem_pool(x_bf, sd, prefix)
    outs = {}
    for si, nb in enumerate(STAGE_BLOCKS[depth]):
        for bi in range(nb):
            first = bi == 0 and si > 0
            ws, ss, hs = block_params(sd, f"{prefix}.res{si + 2}.{bi}", first)
            x = basic_block_bf16(x, ws, ss, hs, 2 if first else 1)
        outs[f"res{si + 2}"] = x
    return outs


def basic_backbone_fpn_bf16(x_bf, sd, depth):
    f = OB16.fpn(resnet_bf16(x_bf, sd, depth), sd)
    return [f[k] for k in ("p3", "p4", "p5", "p6", "p7")]
