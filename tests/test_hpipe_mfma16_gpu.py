"""conv_hpipe_kernel on 16x16x32 MFMAs (csrc/conv_hpipe.hip), pinned to the bf16-storage oracle at every pyramid-level patch shape.

The kernel's K loop, fragment addressing, LDS swizzles and accumulator -> epilogue staging changed with the MFMA shape; the
epilogue after the staging barrier did not.  Each case below runs conv_hpipe through the C ABI on operands that are exact
bf16 values and compares with oracle/bf16.py on the same operands.  Both sides round the same fp32 sum up to summation order,
so (tests/test_bf16_pinned_gpu.py, a conv with no bf16 intermediate): worst element <= 1 bf16 ulp of that element (floor
1e-3 of the tensor's maximum) and <= 1 % of the elements not identical.  A wrong fragment row, tap or channel is a many-ulp
error on some element.

  * plain instantiation (<false>), no GroupNorm statistics: one 3x3 conv per pyramid-level map size (patch shapes 10 x 12,
    9 x 14 with ragged last patches, 13 x 7, 7 x 11), ReLU on and off, Cin 256; res5 conv2 (Cin = Cout = 512);
  * tower layers: <false> with the GroupNorm partials of its epilogue (layer 0) and <true> with the previous layer's GroupNorm +
    ReLU applied to the input halo in LDS (layer 1) over whole five-level pyramids;
  * batch position at the 192-image bench batch: copies of an image give bit-identical tower outputs wherever they sit.
(The GroupNorm-in instantiation always runs with the ReLU on: the FCOS towers are GN + ReLU, the only configuration that fuses.)
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

H, W = 800, 1344
LEVELS = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]


def _cfg():
    from sylph_amd.config import get_default_cfg
    cfg = get_default_cfg()
    cg = cfg.MODEL.META_LEARN.CODE_GENERATOR
    cfg.MODEL.META_LEARN.EPISODIC_LEARNING = True
    cg.CONV_L2_NORM = True
    cg.TOWER_LAYERS = [["GN", "ReLU"], ["GN", "ReLU"]]
    cg.CLS_LAYER = ["", "", 1]
    cg.BIAS_LAYER = ["", "", 1]
    return cfg


def _assert_ulps(got, want, what, max_ulp=1.0, max_frac=0.01):
    got, want = got.float().cpu(), want.float().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = (got - want).abs()
    fl = 1e-3 * float(want.abs().max())
    mag = torch.maximum(torch.maximum(got.abs(), want.abs()), torch.full_like(want, fl))
    ulp = torch.exp2(torch.floor(torch.log2(mag)) - 7)
    frac, worst = float((diff > 0).float().mean()), float((diff / ulp).max())
    print(f"{what}: {frac * 100:.3f} % of elements differ, worst {worst:.2f} bf16 ulp")
    assert worst <= max_ulp and frac <= max_frac, f"{what}: {frac:.4f} of elements differ, worst {worst:.2f} ulp"


# map, channels, batch: >= 90 blocks of two patches, so api_conv.hip pick_conv_route picks conv_hpipe (the
# single-conv entry builds its ops on a scratch context that the per-kernel profile does not see; the tower test below checks
# the kernel names)
CONVS = [((100, 168), 256, 2), ((50, 84), 256, 6), ((25, 42), 256, 24), ((13, 21), 256, 64), ((7, 11), 256, 192),
         ((25, 42), 512, 16)]


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("case", CONVS, ids=[f"{h}x{w}_c{c}" for (h, w), c, _ in CONVS])
def test_plain_conv_pinned_per_patch_shape(case, relu):
    from oracle import bf16 as OB16
    from sylph_amd.engine import Engine
    (h, w), c, B = case
    g = torch.Generator().manual_seed(h * 1000 + c + int(relu))
    x = OB16.r(torch.randn(B, c, h, w, generator=g))
    wt = OB16.r(torch.randn(c, c, 3, 3, generator=g) * (2.0 / (9 * c)) ** 0.5)
    scale, shift = 0.5 + torch.rand(c, generator=g), 0.2 * torch.randn(c, generator=g)
    eng = Engine(None, dtype="bf16")
    y = eng.conv2d(x, wt, scale, shift, 1, 1, relu)
    _, want = OB16.conv_epilogue(x, wt, scale, shift, 1, 1, relu)
    _assert_ulps(y, want, f"conv_hpipe<false> {h}x{w} Cin {c} relu={relu}")


def test_tower_layers_pinned_on_full_pyramid():
    """Layer 0 (<false> + GroupNorm partials) and layer 1 (<true>: GroupNorm + ReLU of layer 0 applied in the halo) of the cls
    tower over all five levels of eight pyramids (the batch at which the launch-size rule fuses the GroupNorm into the next
    conv, as at the production batches), each layer on the operands the HIP graph itself produced."""
    from oracle import bf16 as OB16
    from oracle.head import HEAD_PREFIX
    from sylph_amd import synthetic as Wt
    from sylph_amd.engine import Engine
    B = 8
    sd = Wt.head_state_dict(seed=3, num_classes=60)
    g = torch.Generator().manual_seed(17)
    feats = [OB16.r(torch.randn(B, 256, h, w, generator=g)) for h, w in LEVELS]
    codes = Wt.synthetic_codes(5, seed=4, scale=3.0)
    eng = Engine(_cfg(), dtype="bf16")
    eng.load_state_dict(sd)
    eng.set_debug_taps(True)
    eng.profile_enable(True)
    eng.profile_read()
    eng.import_pyramid(feats, (H, W))
    eng.head(codes["cls_conv"], codes["cls_bias"])
    torch.cuda.synchronize()
    kern = eng.profile_read()["kernels"]
    launches = {k: v["launches"] for k, v in kern.items()}
    assert launches.get("conv_hpipe_kernel<false>", 0) >= 1 and launches.get("conv_hpipe_kernel<true>", 0) >= 1, launches
    eng.profile_enable(False)
    prefix = f"{HEAD_PREFIX}.cls_tower"
    x = feats
    for i in range(2):
        ys, cfs = eng.export_tower(0, i)
        nxt = []
        for l in range(5):
            _, y, cf = OB16.tower_layer(x[l], sd, prefix, i)
            _assert_ulps(ys[l], y, f"cls tower layer {i} level {l}")
            nxt.append(OB16.gn_apply(ys[l].cpu(), cfs[l].cpu()))
        x = nxt


def test_tower_outputs_independent_of_batch_position_at_192():
    """192 images = four distinct pyramids repeated 48 times: every tower layer's output of every copy equals copy 0 bit for bit
    (the K walk is keyed on the patch pair's place inside its image, not in the batch)."""
    from sylph_amd import synthetic as Wt
    from sylph_amd.engine import Engine
    B, D = 192, 4
    sd = Wt.head_state_dict(seed=5, num_classes=60)
    g = torch.Generator(device="cuda").manual_seed(23)
    feats = [torch.randn(D, 256, h, w, generator=g, device="cuda").bfloat16().float().repeat(B // D, 1, 1, 1) for h, w in LEVELS]
    codes = Wt.synthetic_codes(5, seed=4, scale=3.0)
    eng = Engine(_cfg(), dtype="bf16")
    eng.load_state_dict(sd)
    eng.set_debug_taps(True)
    eng.import_pyramid(feats, (H, W))
    del feats
    eng.head(codes["cls_conv"], codes["cls_bias"])
    for t in range(2):
        for i in range(4):
            ys, _ = eng.export_tower(t, i, with_coef=False)
            for l, y in enumerate(ys):
                assert torch.isfinite(y[:D]).all()
                ref = y[:D].repeat(B // D, 1, 1, 1)
                bad = (y != ref).flatten(1).any(dim=1).nonzero().flatten().tolist()
                assert not bad, f"tower {t} layer {i} level {l}: images {bad[:8]} differ from their copy in the first {D}"
            del ys
