"""Test-side restatement of detectron2's ResNeXt backbone (build_resnet_backbone with MODEL.RESNETS.NUM_GROUPS > 1).
TEST INFRASTRUCTURE: the product never imports this file.

detectron2 BottleneckBlock(in, out, bottleneck_channels=mid, stride, num_groups=G, stride_in_1x1):
  conv1 1x1 (stride s1) + FrozenBN + ReLU -> conv2 3x3 pad 1 (stride s3, groups=G) + FrozenBN + ReLU -> conv3 1x1 + FrozenBN,
  + shortcut (1x1 stride + FrozenBN when the shape changes, identity otherwise), ReLU;  (s1, s3) = (stride, 1) if stride_in_1x1
  else (1, stride);  mid of stage s (0 = res2) = G * WIDTH_PER_GROUP << s.

Three forms of the grouped conv / block / backbone:
  * fp32 or float64 F.conv2d(groups=G) (oracle/backbone.py's convs take no groups);
  * an explicit per-group loop: G dense convs on channel slices, concatenated;
  * a bf16 form that rounds where the HIP graph rounds (oracle.bf16.r / fma): every conv epilogue fma(acc, scale, shift) -> bf16,
    the projection folded into conv3's GEMM as api_weights.hip make_c3sc does.
resnext_backbone_fpn / resnext_fcos_head drive oracle.backbone.fpn and oracle.head on the restated features.
"""
from typing import Dict

import torch
import torch.nn.functional as F

from oracle import backbone as OB
from oracle import bf16 as OB16

STAGE_BLOCKS = OB.STAGE_BLOCKS


def grouped_conv_loop(x: torch.Tensor, w: torch.Tensor, groups: int, stride: int = 1, padding: int = 1) -> torch.Tensor:
    """(b) G dense convs, one per channel slice."""
    C = x.shape[1]
    cpg, opg = C // groups, w.shape[0] // groups
    return torch.cat([F.conv2d(x[:, g * cpg:(g + 1) * cpg], w[g * opg:(g + 1) * opg], None, stride=stride, padding=padding)
                      for g in range(groups)], dim=1)


def _conv_bn(x, sd, name, groups=1, stride=1, padding=0, relu=False, loop=False):
    w = sd[name + ".weight"].to(x.dtype)
    if loop and groups > 1:
        y = grouped_conv_loop(x, w, groups, stride, padding)
    else:
        y = F.conv2d(x, w, None, stride=stride, padding=padding, groups=groups)
    sc, sh = OB.bn_scale_shift(sd, name + ".norm")
    y = y * sc.to(x.dtype).view(1, -1, 1, 1) + sh.to(x.dtype).view(1, -1, 1, 1)
    return F.relu(y) if relu else y


def bottleneck(x, sd, prefix, stride, has_shortcut, groups, stride_in_1x1=False, loop=False):
    s1, s3 = (stride, 1) if stride_in_1x1 else (1, stride)
    out = _conv_bn(x, sd, prefix + ".conv1", stride=s1, relu=True)
    out = _conv_bn(out, sd, prefix + ".conv2", groups=groups, stride=s3, padding=1, relu=True, loop=loop)
    out = _conv_bn(out, sd, prefix + ".conv3")
    sc = _conv_bn(x, sd, prefix + ".shortcut", stride=stride) if has_shortcut else x
    return F.relu(out + sc)


def resnet(x, sd, depth, groups, stride_in_1x1=False, loop=False, prefix="backbone.bottom_up") -> Dict[str, torch.Tensor]:
    """{res2..res5} of the ResNeXt bottom-up (stem as detectron2 BasicStem)."""
    x = _conv_bn(x, sd, prefix + ".stem.conv1", stride=2, padding=3, relu=True)
    x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
    outs = {}
    for si, nb in enumerate(STAGE_BLOCKS[depth]):
        for bi in range(nb):
            stride = 2 if (bi == 0 and si > 0) else 1
            x = bottleneck(x, sd, f"{prefix}.res{si + 2}.{bi}", stride, bi == 0, groups, stride_in_1x1, loop)
        outs[f"res{si + 2}"] = x
    return outs


def resnext_backbone_fpn(x, sd, depth, groups, stride_in_1x1=False):
    """images (B,3,H,W) normalised / padded -> [p3..p7] through oracle.backbone.fpn."""
    sdd = {k: v.to(x.dtype) for k, v in sd.items()}
    f = OB.fpn(resnet(x, sdd, depth, groups, stride_in_1x1), sdd)
    return [f[k] for k in ("p3", "p4", "p5", "p6", "p7")]


# ---- bf16 form: rounds where the HIP graph rounds ---------------------------------------------------------------------------------
def conv_epilogue_grouped(x_bf, w, scale, shift, groups, stride=1, padding=1, relu=True):
    acc = F.conv2d(x_bf, OB16.r(w), None, stride=stride, padding=padding, groups=groups)
    v = OB16.fma(acc, scale.view(1, -1, 1, 1), shift.view(1, -1, 1, 1))
    return OB16.r(F.relu(v) if relu else v)


def bottleneck_bf16(x_bf, ws, scales, shifts, stride, groups, stride_in_1x1=False):
    """One block as the HIP graph computes it: t1, t2 stored bf16; conv2 grouped; projection folded into conv3's GEMM."""
    s1, s3 = (stride, 1) if stride_in_1x1 else (1, stride)
    _, t1 = OB16.conv_epilogue(x_bf, ws[0], scales[0], shifts[0], stride=s1, relu=True)
    t2 = conv_epilogue_grouped(t1, ws[1], scales[1], shifts[1], groups, stride=s3)
    if len(ws) > 3 and ws[3] is not None:
        w3f = OB16.r(ws[2] * scales[2].view(-1, 1, 1, 1))
        wsf = OB16.r(ws[3] * scales[3].view(-1, 1, 1, 1))
        acc = F.conv2d(t2, w3f) + F.conv2d(x_bf, wsf, stride=stride)
        return OB16.r(F.relu(acc + (shifts[2] + shifts[3]).view(1, -1, 1, 1)))
    _, y = OB16.conv_epilogue(t2, ws[2], scales[2], shifts[2], relu=True, res_bf=x_bf)
    return y


def block_params(sd, prefix, has_shortcut):
    return OB16.bottleneck_params(sd, prefix, has_shortcut)
