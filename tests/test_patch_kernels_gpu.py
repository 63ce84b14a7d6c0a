"""The bf16 backbone kernels that walk a host-built table of ph x pw patches (add_patch_kernel, BkTile) with hand-written halo
addressing -- bottleneck64_kernel, bottleneck64p_kernel, conv_rw3_kernel -- and the stem kernels with their fixed tiles, pinned to
bf16 ulps on RAGGED maps: partial last rows / columns of patches, maps narrower or lower than one patch, fewer tiles than the eight
XCD walks, tile counts that are no multiple of eight, and more tiles than persistent blocks (a block takes a second patch, and the
prefetch of the next halo meets the end of the table).  tests/test_bf16_pinned_gpu.py holds the same kernels to the same bounds where
the patches divide the map (200 x 336, 100 x 168); an off-by-one in a halo shows on one edge row or column of one ragged patch only.

Every case runs through a parity entry that builds the block as the backbone does (Engine.bottleneck, Engine.basic_block,
Engine.stem_maxpool), on the operands of tests/test_bf16_pinned_gpu.py (_block_params; input bf16(relu(randn))), against the
bf16-storage restatement (oracle/bf16.py, tests/basic_ref.py), and asserts the kernels that ran by name (profile records) and the conv
routes that were built; with a routing override in the environment (SYLPH_CONV_*, SYLPH_SPLIT_*, SYLPH_FUSE_*) the numbers are
checked and the names are not.  The geometry class each case is in the table for is stated beside it and held on the CPU against the
restated pick_patch (tests/patch_ref.py, tests/test_patch_kernels_cpu.py), which also shows that the block bound catches a one-row
and a one-column error at every identity-block shape used here.

Bounds: those of tests/test_bf16_pinned_gpu.py, not tuned -- one block: <= 2 bf16 ulps taken at max(|element|, rms), <= 3 % of the
elements not identical; one conv (the stem): <= 1 ulp of the element (floor 1e-3 of the maximum), <= 1 % not identical.  A failing case
prints the (image, channel, y, x) of its worst elements and where each lies in its patch.

The stem entry launches stem_conv_kernel and stem_pool_kernel itself, outside the profile records and without a route to choose:
there is no kernel name to assert for it."""
import os

import pytest
import torch
import torch.nn.functional as F

import patch_ref as PR
from bf16_ulps import assert_ulps, bf16_rne, conv_epilogue_f64

pytestmark = pytest.mark.gpu

I64 = "igemm 64x128 nbuf2"
IG, RW3 = "conv_igemm_kernel", "conv_rw3_kernel"

# ---- fused res2 blocks, dense: (B, H, W), the patch pick_patch gives, the classes the case is in the table for (patch_ref.classes)
FUSED = [
    ((1, 7, 7), (7, 7), {"exact", "few_tiles"}),                     # one tile that equals the map: 1 tile for an 8-way XCD walk
    ((3, 11, 13), (11, 7), {"ragged_x", "few_tiles"}),               # last column 6 of 7; 6 tiles
    ((2, 17, 23), (9, 12), {"ragged_y", "ragged_x"}),                # ragged 8 / 11; 8 tiles
    ((3, 33, 47), (17, 7), {"ragged_y", "ragged_x", "odd_walk"}),    # the tallest patch, ragged 16 / 5; 42 tiles
    ((1, 3, 130), (3, 19), {"ragged_x", "few_tiles"}),               # the widest patch; 7 tiles
    ((1, 130, 3), (17, 7), {"narrow", "ragged_y"}),                  # a map narrower than the patch
    ((2, 2, 5), (2, 7), {"narrow", "few_tiles"}),                    # a map smaller than any patch
    ((30, 26, 38), (9, 13), {"ragged_y", "ragged_x", "second_patch", "odd_walk"}),  # ragged 8 / 12; 270 tiles
]
# name, Cin, shortcut, kernel
FUSED_BLOCKS = [("identity", 256, False, "bottleneck64_kernel"), ("projection", 64, True, "bottleneck64p_kernel")]

# ---- conv_rw3 at the default knob through Engine.basic_block (128 -> 128, stride 1, identity): (B, H, W), the conv_rw3 patch or None
# (the generic route), classes
RW3_BASIC = [
    ((64, 20, 24), (10, 12), {"exact"}),                             # exactly 30 720 positions; 256 tiles
    ((63, 20, 24), None, {"exact"}),                                 # 30 240 positions: below the launch rule
    ((79, 17, 23), (9, 12), {"ragged_y", "ragged_x", "second_patch", "odd_walk"}),  # ragged 8 / 11; 316 tiles
    ((25, 29, 43), (10, 11), {"ragged_y", "ragged_x", "second_patch", "odd_walk"}),  # ragged 9 / 10; 300 tiles
    ((11, 50, 58), (10, 12), {"ragged_x", "second_patch", "odd_walk"}),             # last column 10; 275 tiles
    ((16, 44, 44), None, {"exact"}),                                 # 30 976 positions, but 11 x 11 fails conv_rw3_patch_ok
]
# ---- ... and through Engine.bottleneck (512 / 128 / 512 identity): pick_block_route hands conv2 to conv_rw3 (Conv2Form::rw3)
RW3_BOTTLENECK = ((32, 26, 38), (9, 13), {"ragged_y", "ragged_x", "second_patch"})  # ragged 8 / 12; 288 tiles

STEM = [(2, 64, 96), (1, 75, 118), (3, 33, 47), (1, 9, 11)]
STEM_TILE = (8, 16)  # stem_conv_kernel's output tile


def _id(c):
    return "B%d_%dx%d" % c[0] if isinstance(c[0], tuple) else "B%d_%dx%d" % c


def _overrides():
    return sorted(k for k in os.environ if k.startswith(("SYLPH_CONV_", "SYLPH_SPLIT_", "SYLPH_FUSE_")))


def bottleneck_operands(shape, cin, mid, cout, shortcut):
    """Input and parameters of one bottleneck case (shared with the CPU sensitivity test)."""
    from oracle import bf16 as OB16
    from test_bf16_pinned_gpu import _block_params
    B, h, w = shape
    g = torch.Generator().manual_seed(cin + mid + 1000 * B + 37 * h + w)
    x = OB16.r(F.relu(torch.randn(B, cin, h, w, generator=g)))
    return (x,) + _block_params(g, cin, mid, cout, shortcut)


def basic_block_operands(shape, ch=128):
    """Input and parameters of one identity BasicBlock case: two 3x3 layers drawn as _block_params draws its layers (He weights, scale
    0.5 + rand, shift 0.2 * randn), no shortcut."""
    from oracle import bf16 as OB16
    B, h, w = shape
    g = torch.Generator().manual_seed(ch + 1000 * B + 37 * h + w)
    x = OB16.r(F.relu(torch.randn(B, ch, h, w, generator=g)))
    ws = [torch.randn(ch, ch, 3, 3, generator=g) * (2.0 / (ch * 9)) ** 0.5 for _ in range(2)]
    scales = [0.5 + torch.rand(ch, generator=g) for _ in range(2)]
    shifts = [0.2 * torch.randn(ch, generator=g) for _ in range(2)]
    return x, ws + [None], scales + [None], shifts + [None]


def _engine():
    from sylph_amd.engine import Engine
    eng = Engine(None, dtype="bf16")
    eng.profile_enable(True)
    return eng


def _forms(eng, what):
    kernels, routes = eng.profile_read()["kernels"], eng.conv_routes()
    print(f"{what}: kernels {dict((k, v['launches']) for k, v in kernels.items())}, conv routes {routes}")
    return kernels, routes


def worst_elements(got, want, floor, patch, n=8):
    """The n elements furthest from `want` in bf16 ulps (tests/bf16_ulps.py ulps): (ulps, image, channel, y, x, where in its patch)."""
    got, want = got.float().cpu(), want.float().cpu()
    fl = 1e-3 * float(want.abs().max()) if floor == "max" else float(want.pow(2).mean().sqrt())
    mag = torch.maximum(torch.maximum(got.abs(), want.abs()), torch.full_like(want, fl)).clamp_min(2.0 ** -126)
    err = (got - want).abs() / torch.exp2(torch.floor(torch.log2(mag)) - 7)
    B, C, H, W = want.shape
    top = torch.topk(err.flatten(), min(n, err.numel()))
    out = []
    for e, i in zip(top.values.tolist(), top.indices.tolist()):
        if e == 0:
            break
        b, c, y, x = i // (C * H * W), i // (H * W) % C, i // W % H, i % W
        out.append((e, b, c, y, x, PR.patch_edges(y, x, patch[0], patch[1], H, W) or "interior"))
    return out


def _pin(got, want, what, patch, **bound):
    """assert_ulps; a failure first prints where the worst elements lie in their patches."""
    try:
        assert_ulps(got, want, what, **bound)
    except AssertionError:
        print(f"{what}: worst elements, {patch[0]} x {patch[1]} patches")
        for e, b, c, y, x, where in worst_elements(got, want, bound.get("floor", "max"), patch):
            print(f"  {e:9.2f} ulp at image {b} channel {c} (y, x) = ({y}, {x}): {where}")
        raise


BLOCK_BOUND = dict(max_ulp=2.0, max_frac=0.03, floor="rms")


@pytest.mark.parametrize("block", FUSED_BLOCKS, ids=[b[0] for b in FUSED_BLOCKS])
@pytest.mark.parametrize("case", FUSED, ids=[_id(c) for c in FUSED])
def test_fused_res2_blocks_pinned_on_ragged_maps(case, block):
    """bottleneck64_kernel (256 / 64 / 256 identity) and bottleneck64p_kernel (64 / 64 / 256 with the projection folded into conv3): ONE
    launch of the one kernel, no conv route, against oracle.bf16.bottleneck."""
    from oracle import bf16 as OB16
    shape, patch, _ = case
    name, cin, shortcut, kernel = block
    what = f"{kernel} {_id(shape)}"
    x, ws, scales, shifts = bottleneck_operands(shape, cin, 64, 256, shortcut)
    eng = _engine()
    y = eng.bottleneck(x, ws, scales, shifts, 1)
    kernels, routes = _forms(eng, what)
    _pin(y, OB16.bottleneck(x, ws, scales, shifts, 1), what, patch, **BLOCK_BOUND)
    if not _overrides():
        assert list(kernels) == [kernel] and kernels[kernel]["launches"] == 1 and routes == [], (kernels, routes)


def _skip_if_rw3_knob():
    if "SYLPH_CONV_RW3" in os.environ:
        pytest.skip("SYLPH_CONV_RW3 is set (read once per process): these cases pin the launch rule of the default")


@pytest.mark.parametrize("case", RW3_BASIC, ids=[_id(c) for c in RW3_BASIC])
def test_conv_rw3_pinned_on_ragged_maps_at_the_default_knob(case):
    """A 128 -> 128 identity BasicBlock (the R-18 / R-34 res3 block): conv1 on conv_rw3_kernel where the launch has at least 256 * 120
    positions and its patch passes conv_rw3_patch_ok, on conv_igemm otherwise; conv2 (with the residual) always on the generic route.
    The launches reach 30 720 positions by batch; against tests/basic_ref.py basic_block_bf16."""
    from tests import basic_ref as BR
    _skip_if_rw3_knob()
    shape, patch, _ = case
    B, h, w = shape
    what = f"BasicBlock 128 {_id(shape)}"
    x, ws, scales, shifts = basic_block_operands(shape)
    eng = _engine()
    y = eng.basic_block(x, ws, scales, shifts, 1)
    kernels, routes = _forms(eng, what)
    _pin(y, BR.basic_block_bf16(x, ws, scales, shifts, 1), what, patch or PR.pick_patch(h, w), **BLOCK_BOUND)
    if _overrides():
        return
    if patch:
        assert list(kernels) == [RW3, IG] and kernels[RW3]["launches"] == 1 and kernels[IG]["launches"] == 1 and routes == [I64], (kernels, routes)
    else:
        assert list(kernels) == [IG] and kernels[IG]["launches"] == 2 and routes == [I64, I64], (kernels, routes)


def test_conv_rw3_through_the_bottleneck_block_route_on_a_ragged_map():
    """A 512 / 128 / 512 identity bottleneck (res3) at 32 x 26 x 38: pick_block_route hands conv2 to conv_rw3 (9 x 13 patches, ragged 8 / 12,
    288 tiles).  31 616 positions: conv1 (247 128-row blocks < 1 024: 64-row tiles; N = 128 at stride 1 stays off conv_pw; 512 tiles > 400:
    two LDS stages) and conv3 (same-geometry residual with 247 M tiles < conv_spw's 512; 2 048 tiles) both run conv_igemm on 64 x 128."""
    from oracle import bf16 as OB16
    _skip_if_rw3_knob()
    shape, patch, _ = RW3_BOTTLENECK
    what = f"bottleneck 512/128/512 {_id(shape)}"
    x, ws, scales, shifts = bottleneck_operands(shape, 512, 128, 512, False)
    eng = _engine()
    y = eng.bottleneck(x, ws, scales, shifts, 1)
    kernels, routes = _forms(eng, what)
    _pin(y, OB16.bottleneck(x, ws, scales, shifts, 1), what, patch, **BLOCK_BOUND)
    if not _overrides():
        assert list(kernels) == [IG, RW3] and kernels[RW3]["launches"] == 1 and kernels[IG]["launches"] == 2 and routes == [I64, I64], (kernels, routes)


@pytest.mark.parametrize("shape", STEM, ids=[_id(c) for c in STEM])
def test_stem_kernels_pinned_on_ragged_maps(shape):
    """stem_conv_kernel (8 x 16 output tiles) on maps with partial tiles in both directions and on one smaller than a tile, against
    float64 on the bf16 operands with ONE rounding; stem_pool_kernel bit-equal to the max-pool of the kernel's own stem output."""
    B, H, W = shape
    g = torch.Generator().manual_seed(5 + 1000 * B + 37 * H + W)
    x = (torch.randn(B, 3, H, W, generator=g) * 60.0).bfloat16().float()
    w = (torch.randn(64, 3, 7, 7, generator=g) * (2.0 / 147) ** 0.5 / 60.0).bfloat16().float()
    scale, shift = 0.5 + torch.rand(64, generator=g), 0.2 * torch.randn(64, generator=g)
    stem, pool = _engine().stem_maxpool(x, w, scale, shift)
    _pin(stem, bf16_rne(conv_epilogue_f64(x, w, scale, shift, 2, 3, True)), f"stem_conv_kernel {_id(shape)}", STEM_TILE)
    assert torch.equal(pool.cpu(), F.max_pool2d(stem.cpu(), 3, 2, 1)), f"stem_pool_kernel {_id(shape)}: differs from pooling the stand-alone stem output"
