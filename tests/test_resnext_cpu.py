"""ResNeXt backbones (MODEL.RESNETS.NUM_GROUPS > 1) on the host: the config keys map onto the C struct and unsupported combinations
still raise, the synthetic ResNeXt checkpoint has detectron2's shapes without disturbing the default one, and the test-side
restatements of the grouped block agree with each other and with an independent implementation (transformers' RegNetXLayer)."""
import pytest
import torch
import torch.nn.functional as F

from tests import resnext_ref as XR


def _cfg(groups, wpg, depth=101, stride_in_1x1=False):
    from sylph_amd.config import get_default_cfg
    cfg = get_default_cfg()
    r = cfg.MODEL.RESNETS
    r.DEPTH, r.NUM_GROUPS, r.WIDTH_PER_GROUP, r.STRIDE_IN_1X1 = depth, groups, wpg, stride_in_1x1
    return cfg


@pytest.mark.parametrize("groups,wpg,depth", [(32, 8, 101), (32, 4, 50), (64, 4, 101), (32, 8, 152)])
@pytest.mark.parametrize("stride_in_1x1", [False, True])
def test_config_maps_resnext(groups, wpg, depth, stride_in_1x1):
    from sylph_amd.engine import config_from_cfg
    sc = config_from_cfg(_cfg(groups, wpg, depth, stride_in_1x1))
    assert (sc.num_groups, sc.width_per_group, sc.resnet_depth, sc.stride_in_1x1) == (groups, wpg, depth, int(stride_in_1x1))


def test_config_default_is_plain_resnet():
    from sylph_amd.config import get_default_cfg
    from sylph_amd.engine import config_from_cfg
    sc = config_from_cfg(get_default_cfg())
    assert (sc.num_groups, sc.width_per_group) == (1, 64)


@pytest.mark.parametrize("groups,wpg", [(32, 2), (4, 32), (8, 16), (32, 3), (3, 64), (20, 8), (32, 6)])
def test_config_refuses_uncovered_widths(groups, wpg):
    """per-group width 2 (below 4), 128 or more at res5 (16 << 3, 32 << 3), non-powers of two, G * W not a multiple of 64"""
    from sylph_amd.engine import config_from_cfg
    with pytest.raises(NotImplementedError, match="NUM_GROUPS"):
        config_from_cfg(_cfg(groups, wpg))


@pytest.mark.parametrize("key,value,match", [("DEFORM_ON_PER_STAGE", [False, True, True, True], "DEFORM_ON_PER_STAGE"),
                                             ("RES5_DILATION", 2, "RES5_DILATION")])
def test_config_still_refuses_other_backbone_branches(key, value, match):
    from sylph_amd.engine import config_from_cfg
    cfg = _cfg(32, 8)
    cfg.MODEL.RESNETS[key] = value
    with pytest.raises(NotImplementedError, match=match):
        config_from_cfg(cfg)


def test_synthetic_resnext_keys_have_detectron2_shapes():
    from sylph_amd import synthetic as W
    sd = W.backbone_state_dict(0, depth=50, num_groups=32, width_per_group=4)
    base = W.backbone_state_dict(0, depth=50)
    assert set(sd) == set(base)
    cin = 64
    for si, nb in enumerate(XR.STAGE_BLOCKS[50]):
        mid, cout = (32 * 4) << si, 256 << si
        for bi in range(nb):
            q = f"backbone.bottom_up.res{si + 2}.{bi}"
            assert tuple(sd[q + ".conv1.weight"].shape) == (mid, cin, 1, 1)
            assert tuple(sd[q + ".conv2.weight"].shape) == (mid, mid // 32, 3, 3)
            assert tuple(sd[q + ".conv3.weight"].shape) == (cout, mid, 1, 1)
            assert tuple(sd[q + ".conv2.norm.running_var"].shape) == (mid,)
            if bi == 0:
                assert tuple(sd[q + ".shortcut.weight"].shape) == (cout, cin, 1, 1)
            cin = cout
    for k in base:
        if ".res" not in k:
            assert sd[k].shape == base[k].shape, k


def test_default_synthetic_dict_unchanged():
    """the default call draws exactly the tensors it drew before the ResNeXt option existed (one generator, same order)"""
    import math
    from sylph_amd import synthetic as W
    g = torch.Generator().manual_seed(0)
    want = torch.randn(64, 3, 7, 7, generator=g) * math.sqrt(2.0 / 147) / 64.0
    sd = W.backbone_state_dict(0, depth=50)
    assert torch.equal(sd["backbone.bottom_up.stem.conv1.weight"], want)
    explicit = W.backbone_state_dict(0, depth=50, num_groups=1, width_per_group=64)
    assert all(torch.equal(sd[k], explicit[k]) for k in sd)
    assert tuple(sd["backbone.bottom_up.res4.5.conv2.weight"].shape) == (256, 256, 3, 3)


@pytest.mark.parametrize("groups,cpg,stride", [(32, 4, 1), (16, 8, 2), (4, 16, 1), (2, 32, 2), (2, 64, 1)])
def test_grouped_conv_restatements_agree(groups, cpg, stride):
    g = torch.Generator().manual_seed(groups * cpg + stride)
    C = groups * cpg
    x = torch.randn(2, C, 9, 7, generator=g, dtype=torch.float64)
    w = torch.randn(C, cpg, 3, 3, generator=g, dtype=torch.float64)
    a = F.conv2d(x, w, None, stride=stride, padding=1, groups=groups)
    b = XR.grouped_conv_loop(x, w, groups, stride)
    assert float((a - b).abs().max()) <= 1e-12
    # an explicit multiply-accumulate at a few output positions
    xp = F.pad(x, (1, 1, 1, 1))
    for (n, o, oy, ox) in [(0, 0, 0, 0), (1, C - 1, a.shape[2] - 1, a.shape[3] - 1), (0, C // 2 + 1, 1, 2)]:
        gi = o // cpg
        patch = xp[n, gi * cpg:(gi + 1) * cpg, oy * stride:oy * stride + 3, ox * stride:ox * stride + 3]
        assert abs(float((patch * w[o]).sum()) - float(a[n, o, oy, ox])) <= 1e-12


def test_block_and_backbone_restatements_agree():
    from sylph_amd import synthetic as W
    sd = {k: v.double() for k, v in W.backbone_state_dict(3, depth=50, num_groups=32, width_per_group=4).items()}
    x = torch.randn(1, 3, 64, 96, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    a = XR.resnet(x, sd, 50, 32, stride_in_1x1=False)
    b = XR.resnet(x, sd, 50, 32, stride_in_1x1=False, loop=True)
    for k in a:
        assert float((a[k] - b[k]).abs().max()) <= 1e-12 * max(1.0, float(a[k].abs().max())), k
    assert tuple(a["res5"].shape) == (1, 2048, 2, 3)
    # the bf16 block form tracks the exact one
    x2 = OB16r(torch.relu(torch.randn(1, 256, 12, 10, generator=torch.Generator().manual_seed(2))))
    ws, ss, hs = XR.block_params({k: v.float() for k, v in sd.items()}, "backbone.bottom_up.res3.0", True)
    exact = XR.bottleneck(x2.double(), sd, "backbone.bottom_up.res3.0", 2, True, 32)
    got = XR.bottleneck_bf16(x2, ws, ss, hs, 2, 32)
    assert float((got.double() - exact).abs().max()) <= 0.05 * float(exact.abs().max())


def OB16r(t):
    from oracle import bf16 as OB16
    return OB16.r(t)


@pytest.mark.parametrize("cin,out,stride,hw", [(64, 256, 1, (9, 11)), (256, 512, 2, (10, 13)), (512, 512, 1, (6, 5))])
def test_regnetx_layer_is_a_resnext_block(cin, out, stride, hw):
    """transformers' RegNetXLayer with groups_width = the stage's per-group width is a 32x8d ResNeXt block with STRIDE_IN_1X1 False
    (mid == out at every 32x8d stage); BatchNorm2d in eval mode = FrozenBN."""
    pytest.importorskip("transformers")
    from transformers import RegNetConfig
    from transformers.models.regnet.modeling_regnet import RegNetXLayer
    torch.manual_seed(cin + out)
    mid, groups = out, 32
    layer = RegNetXLayer(RegNetConfig(groups_width=mid // groups, hidden_act="relu"), cin, out, stride=stride).eval()
    g = torch.Generator().manual_seed(cin * 7 + out)
    sd, q = {}, "blk"
    mods = {"conv1": layer.layer[0], "conv2": layer.layer[1], "conv3": layer.layer[2]}
    if stride != 1 or cin != out:
        mods["shortcut"] = layer.shortcut
    for name, m in mods.items():
        w = torch.randn(m.convolution.weight.shape, generator=g) * (2.0 / m.convolution.weight[0].numel()) ** 0.5
        bn = {"weight": torch.rand(w.shape[0], generator=g) + 0.5, "bias": 0.1 * torch.randn(w.shape[0], generator=g),
              "running_mean": 0.1 * torch.randn(w.shape[0], generator=g), "running_var": torch.rand(w.shape[0], generator=g) + 0.5}
        with torch.no_grad():
            m.convolution.weight.copy_(w)
            for k, v in bn.items():
                getattr(m.normalization, k).copy_(v)
        sd[f"{q}.{name}.weight"] = w
        for k, v in bn.items():
            sd[f"{q}.{name}.norm.{k}"] = v
    x = torch.relu(torch.randn(2, cin, *hw, generator=g))
    with torch.no_grad():
        want = layer(x)
    got = XR.bottleneck(x, sd, q, stride, "shortcut" in mods, groups, stride_in_1x1=False)
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))
