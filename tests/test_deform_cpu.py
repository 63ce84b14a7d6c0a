"""MODEL.FCOS.USE_DEFORMABLE on the host: the two test-side restatements of the modulated deformable conv agree, the config key maps
onto the C struct, and the synthetic deformable checkpoint has the DFConv2d key set without disturbing any existing key."""
import pytest
import torch
import torch.nn.functional as F

from tests import deform_ref as DR


def _maps(seed, B=2, C=3, H=5, W=6):
    g = torch.Generator().manual_seed(seed)
    return g, torch.randn(B, C, H, W, generator=g, dtype=torch.float64)


def _om(g, B, H, W, kind):
    om = torch.zeros(B, 27, H, W, dtype=torch.float64)
    om[:, 18:] = torch.randn(B, 9, H, W, generator=g, dtype=torch.float64)
    if kind == "fractional":
        om[:, :18] = 2.0 * torch.randn(B, 18, H, W, generator=g, dtype=torch.float64)
    elif kind == "integer":
        om[:, :18] = torch.randint(-3, 4, (B, 18, H, W), generator=g).double()
    elif kind == "border":  # samples landing exactly on -1 and on H / W
        ys = torch.arange(H, dtype=torch.float64).view(1, H, 1)
        xs = torch.arange(W, dtype=torch.float64).view(1, 1, W)
        for j in range(9):
            ky, kx = divmod(j, 3)
            pick = torch.randint(0, 4, (B, H, W), generator=g)
            ty = torch.where(pick == 0, torch.full_like(pick, -1).double(), torch.where(pick == 1, torch.full_like(pick, H).double(),
                                                                                          0.5 * torch.ones_like(pick).double()))
            tx = torch.where(pick == 2, torch.full_like(pick, -1).double(), torch.where(pick == 3, torch.full_like(pick, W).double(),
                                                                                          0.25 * torch.ones_like(pick).double()))
            om[:, 2 * j] = ty - (ys - 1 + ky)
            om[:, 2 * j + 1] = tx - (xs - 1 + kx)
    elif kind == "far":
        om[:, :18] = 40.0 * torch.randn(B, 18, H, W, generator=g, dtype=torch.float64)
    elif kind == "zero":
        pass
    return om


@pytest.mark.parametrize("kind", ["fractional", "integer", "border", "far", "zero"])
def test_loop_and_grid_sample_restatements_agree(kind):
    g, x = _maps(11 + len(kind))
    B, C, H, W = x.shape
    om = _om(g, B, H, W, kind)
    w = torch.randn(4, C, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(4, generator=g, dtype=torch.float64)
    a = DR.deform_conv_loop(x, om, w, b)
    gs = DR.deform_conv_grid_sample(x, om, w, b)
    assert float((a - gs).abs().max()) <= 1e-12
    if kind == "far":  # (almost) every sample off the map: only the bias survives where all nine taps left
        assert torch.isfinite(a).all()


def test_zero_offsets_unit_mask_is_conv2d():
    g, x = _maps(5, B=1, C=4, H=7, W=4)
    om = torch.zeros(1, 27, 7, 4, dtype=torch.float64)
    om[:, 18:] = 60.0  # sigmoid == 1 in float64
    w = torch.randn(3, 4, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(3, generator=g, dtype=torch.float64)
    want = F.conv2d(x, w, b, padding=1)
    assert float((DR.deform_conv_loop(x, om, w, b) - want).abs().max()) <= 1e-12
    assert float((DR.deform_conv_grid_sample(x, om, w, b) - want).abs().max()) <= 1e-12


def test_bf16_restatement_tracks_the_exact_one():
    g, x = _maps(7, B=1, C=8, H=6, W=9)
    x = x.float().bfloat16().double()
    om = _om(g, 1, 6, 9, "fractional")
    w = torch.randn(5, 8, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(5, generator=g, dtype=torch.float64)
    exact = DR.deform_conv_grid_sample(x, om.float().double(), w.float().bfloat16().double(), b)
    got = DR.deform_conv_bf16(x, om.float(), w, b.float())
    assert float((got - exact).abs().max()) <= 0.02 * float(exact.abs().max())
    # no bf16 rounding: the fp32 A operand agrees with the float64 loop to fp32 precision
    A = DR.sample_fp32(x, om.float(), round_bf16=False)
    y = DR.deform_conv_from_samples(A, w.float().bfloat16().double(), b)
    assert float((y - exact).abs().max()) <= 1e-5 * float(exact.abs().max())


def test_config_maps_use_deformable():
    from sylph_amd.config import get_default_cfg
    from sylph_amd.engine import config_from_cfg
    cfg = get_default_cfg()
    assert config_from_cfg(cfg).tower_deformable == 0
    cfg.MODEL.FCOS.USE_DEFORMABLE = True
    sc = config_from_cfg(cfg)
    assert sc.tower_deformable == 1
    # the backbone DCN stays out of scope
    cfg.MODEL.RESNETS.DEFORM_ON_PER_STAGE = [False, True, True, True]
    with pytest.raises(NotImplementedError):
        config_from_cfg(cfg)


@pytest.mark.parametrize("norm", ["GN", "none"])
def test_synthetic_deformable_head_keys(norm):
    from sylph_amd import synthetic as Wt
    p = "proposal_generator.fcos_head"
    base = Wt.head_state_dict(seed=3, norm=norm)
    assert Wt.head_state_dict(seed=3, norm=norm, deformable=False).keys() == base.keys()
    dfm = Wt.head_state_dict(seed=3, norm=norm, deformable=True)
    k = (3 if norm == "GN" else 2) * 3
    gone, new = set(), set()
    for t in ("cls_tower", "bbox_tower"):
        gone |= {f"{p}.{t}.{k}.weight", f"{p}.{t}.{k}.bias"}
        new |= {f"{p}.{t}.{k}.offset.weight", f"{p}.{t}.{k}.offset.bias", f"{p}.{t}.{k}.conv.weight", f"{p}.{t}.{k}.conv.bias"}
        assert dfm[f"{p}.{t}.{k}.offset.weight"].shape == (27, 256, 3, 3)
        assert dfm[f"{p}.{t}.{k}.offset.bias"].shape == (27,)
        assert dfm[f"{p}.{t}.{k}.conv.weight"].shape == (256, 256, 3, 3)
        assert dfm[f"{p}.{t}.{k}.conv.bias"].shape == (256,)
    assert set(dfm) == (set(base) - gone) | new
    for key in set(base) - gone:
        assert torch.equal(dfm[key], base[key]), key
    # offsets span a few pixels on a GroupNorm + ReLU input; mask logits are not saturated
    x = F.relu(torch.randn(1, 256, 12, 16, generator=torch.Generator().manual_seed(0)))
    om = F.conv2d(x, dfm[f"{p}.cls_tower.{k}.offset.weight"], dfm[f"{p}.cls_tower.{k}.offset.bias"], padding=1)
    off = om[:, :18]
    assert 1.0 < float(off.std()) < 4.0 and float(off.abs().max()) > 4.0
    assert 0.5 < float(om[:, 18:].std()) < 3.0


def test_checkpoint_passes_deformable_keys():
    from sylph_amd import checkpoint as CK
    from sylph_amd import synthetic as Wt
    sd = Wt.head_state_dict(seed=3, deformable=True)
    out = CK.to_reference_keys(sd)
    for key, v in sd.items():
        assert torch.equal(out[key], v), key
