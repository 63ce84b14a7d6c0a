"""Every conv route of pick_conv_route (csrc/api_conv.hip) that sylph_conv2d can reach, on both sides of each launch-size threshold,
pinned to a float64 reference at bf16-ulp level -- and each case asserts the route that ran (Engine.conv_routes(): one record per
add_conv while profiling is on), so a retuned threshold that moves a case onto another kernel fails here by name instead of silently
moving the coverage.

Reference: x, w and the residual rounded to bf16 (the operands the kernel stores), scale / shift as fp32 values; conv and epilogue
acc * scale + shift (+ res), ReLU in float64; ONE bf16 RNE rounding.  The kernel sums the same exact bf16 products in fp32 and rounds
once, so the only difference is a 1-ulp flip where the fp32 sum sits on the other side of a rounding boundary: worst element <= 1 bf16
ulp (floor 1e-3 of the tensor maximum), <= 1 % of elements not identical (tests/test_bf16_pinned_gpu.py, single-conv kernels).

fp32 modes (one case per geometry class), per element, with S = sum |x * w * scale| + |shift| + |res| (float64) and u = 2^-24:
  * "f32": products and partial sums rounded to fp32, epilogue in fp32: K + 3 roundings of mean-zero independent error, each at most
    u relative to a partial sum <= S.  The probabilistic bound of Higham & Mary (SIAM J. Sci. Comput. 41(5), 2019) gives
    |err| <= lam * sqrt(K + 3) * u * S with probability >= 1 - 2 exp(-lam^2 / 2) per element; lam = 8: < 3e-14 per element, < 1e-6
    over all elements of the table.
  * "f32s": each operand is split into bf16 hi + lo, which keeps 16 mantissa bits: |x - x_hi - x_lo| <= 2^-17 |x| (the statement of
    tests/test_split_mode_gpu.py), the same for w; the dropped parts are at most (2 * 2^-17 + 2^-34) |x w| per product, summed with
    their signs in the worst case: 2^-16 * S on top of the fp32 bound above.
"""
import os

import pytest
import torch

from bf16_ulps import assert_ulps, bf16_rne, conv_epilogue_f64

# The environment knobs that move pick_conv_route: with any of them set, the routes below are not the ones the defaults pick.
OVERRIDE_PREFIXES = ("SYLPH_CONV_", "SYLPH_SPLIT_")

# B, Cin, H, W, Cout, k, stride, relu, residual, expected route (pad = k // 2)
CASES = [
    # conv_hpipe: >= 90 blocks of 256 x 256 over patch pairs, no residual, Cout % 256 == 0, 3x3 s1
    (1, 64, 146, 146, 256, 3, 1, True, False, "igemm 64x128 nbuf2"),        # 88 blocks
    (1, 64, 148, 148, 256, 3, 1, True, False, "hpipe 256x256"),             # 90 blocks
    (1, 256, 148, 148, 256, 3, 1, False, False, "hpipe 256x256"),           # deep K (2304)
    (3, 64, 160, 160, 256, 3, 1, True, False, "igemm_halo 128x128"),        # 300 blocks: in the 257-319 gap
    (4, 64, 180, 180, 256, 3, 1, True, False, "igemm_halo 128x128"),        # 520 blocks in 3 rounds: fill rule fails
    (4, 64, 200, 200, 256, 3, 1, True, False, "hpipe 256x256"),             # 640 blocks: fill rule passes
    (1, 64, 100, 100, 512, 3, 1, True, False, "igemm 64x128 nbuf2"),        # Cout 512: 80 blocks
    (1, 64, 106, 106, 512, 3, 1, False, False, "hpipe 256x256"),            # Cout 512: 96 blocks
    # conv_igemm halo tiles: 128-row tiles, 3x3 s1, patches waste <= 1/2 of the launch; BN 128 / 64 / 32
    (2, 64, 256, 256, 128, 3, 1, True, False, "igemm_halo 128x128"),
    (1100, 64, 10, 13, 128, 3, 1, False, False, "igemm 128x128"),           # 10 x 13 maps: two patches of 128 for 130 positions
    (2, 64, 256, 256, 80, 3, 1, False, False, "igemm_halo 128x128"),        # Cout 80: 48 pad channels in the tile
    (2, 64, 256, 256, 64, 3, 1, True, False, "igemm_halo 128x64"),
    (1100, 64, 10, 13, 64, 3, 1, True, False, "igemm 128x64"),
    (1, 64, 96, 96, 20, 3, 1, False, False, "igemm_halo 128x32"),
    (1, 512, 96, 96, 20, 3, 1, True, False, "igemm_halo 128x32"),           # deep K (4608)
    (200, 64, 10, 13, 20, 3, 1, False, False, "igemm 128x32"),
    (2, 64, 40, 40, 6, 3, 1, False, False, "igemm_halo 128x32"),
    # conv_spw: same-geometry residual, K 128 / 256 / 512, from 512 M tiles of 128 rows
    (7, 128, 73, 128, 512, 1, 1, True, True, "igemm 128x128"),             # 511 M tiles
    (4, 128, 128, 128, 512, 1, 1, True, True, "spw 128x256"),               # 512
    (7, 256, 73, 128, 512, 1, 1, False, True, "igemm 128x128"),
    (4, 256, 128, 128, 512, 1, 1, False, True, "spw 128x256"),
    (7, 512, 73, 128, 512, 1, 1, True, True, "igemm 128x128"),
    (4, 512, 128, 128, 512, 1, 1, True, True, "spw 128x256"),
    # conv_pw: no residual, from 256 tiles; Cout 128 only strided
    (1, 128, 128, 255, 256, 1, 1, True, False, "igemm 64x128 nbuf2"),       # 255 tiles
    (1, 128, 128, 256, 256, 1, 1, True, False, "pw 128x256"),               # 256
    (1, 1024, 128, 256, 256, 1, 1, False, False, "pw 128x256"),             # deep K
    (1, 256, 512, 512, 128, 1, 2, True, False, "pw 256x128"),               # stride 2
    # plain conv_igemm: 128-row tiles; 64-row tiles on three LDS stages up to 400 tiles, two from 401; 64 x 64 up to 160 64 x 128 tiles
    (1, 64, 512, 512, 256, 3, 2, True, False, "igemm 128x128"),             # stride 2, 1024 128-row blocks
    (1, 64, 160, 160, 128, 3, 1, True, False, "igemm 64x128 nbuf3"),        # 400 tiles
    (1, 64, 401, 64, 128, 3, 1, True, False, "igemm 64x128 nbuf2"),         # 401
    (1, 64, 80, 128, 128, 3, 1, True, False, "igemm 64x64 nbuf3"),          # 160 64 x 128 tiles -> 64 x 64
    (1, 64, 92, 112, 128, 3, 1, True, False, "igemm 64x128 nbuf3"),         # 161
    (1, 64, 100, 100, 80, 3, 1, False, False, "igemm 64x64 nbuf3"),         # Cout 80
    (2, 256, 160, 160, 128, 1, 2, True, False, "igemm 64x128 nbuf3"),       # 1x1 stride 2
    (2, 256, 13, 21, 6, 3, 2, False, False, "igemm 128x32"),                # Cout 6, 3x3 stride 2
    (1, 64, 64, 64, 256, 1, 1, True, True, "igemm 64x64 nbuf3"),            # 1x1 + residual, K 64
    (1, 1024, 25, 42, 256, 3, 1, True, False, "igemm 64x64 nbuf3"),         # 68 tiles at 144 K-slices
    # split K (fp32 partial planes + finish pass): <= 64 tiles at >= 32 K-slices, < 64 at >= 64
    (1, 256, 64, 64, 64, 3, 1, True, False, "igemm_splitk 64x64 nbuf2 ks8"),  # 64 tiles, 36 slices
    (1, 256, 64, 65, 64, 3, 1, True, False, "igemm 64x64 nbuf3"),             # 65
    (1, 256, 64, 64, 64, 3, 1, True, True, "igemm_splitk 64x64 nbuf2 ks8"),   # residual in the finish pass
    (1, 512, 63, 64, 64, 3, 1, False, False, "igemm_splitk 64x64 nbuf2 ks8"), # 63 tiles, 72 slices
    (1, 512, 64, 65, 64, 3, 1, False, False, "igemm 64x64 nbuf3"),            # 65
    (1, 2048, 64, 64, 64, 1, 1, False, True, "igemm_splitk 64x64 nbuf2 ks8"), # 1x1, 32 slices, residual
    (1, 2048, 64, 64, 64, 1, 1, True, False, "igemm_splitk 64x64 nbuf2 ks8"),
    (1, 2048, 64, 65, 64, 1, 1, False, True, "igemm 64x64 nbuf3"),
    (1, 512, 13, 21, 256, 3, 1, True, False, "igemm_splitk 64x64 nbuf2 ks8"),  # FPN P5-like: 20 tiles
]

KERNEL_OF = {"hpipe": "conv_hpipe_kernel<false>", "pw": "conv_pw_kernel", "spw": "conv_spw_kernel"}


def _case_id(c):
    B, cin, h, w, cout, k, s, relu, res, route = c
    return f"B{B}_{cin}x{h}x{w}_to{cout}_k{k}s{s}{'_res' if res else ''}{'_relu' if relu else ''}"


def _overrides():
    return sorted(k for k in os.environ if k.startswith(OVERRIDE_PREFIXES))


def _operands(case, bf16):
    B, cin, h, w, cout, k, s, relu, use_res, _ = case
    g = torch.Generator().manual_seed(B * 7919 + cin * 31 + h * 7 + w + cout * 3 + k + s)
    x = torch.randn(B, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    scale = torch.rand(cout, generator=g) + 0.5
    shift = torch.randn(cout, generator=g) * 0.1
    ho, wo = (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1
    res = torch.randn(B, cout, ho, wo, generator=g) if use_res else None
    if bf16:
        x, wt = x.bfloat16().float(), wt.bfloat16().float()
        res = res.bfloat16().float() if res is not None else None
    return x, wt, scale, shift, res


def test_case_table_reaches_every_route():
    """The table's cases together reach every ConvKind and both LDS-stage counts of the 64-row tiles (each case asserts that its
    route is the one that ran)."""
    routes = [c[-1] for c in CASES]
    kinds = {r.split()[0] for r in routes}
    assert kinds == {"hpipe", "igemm_halo", "pw", "spw", "igemm_splitk", "igemm"}, kinds
    assert any("nbuf2" in r and r.startswith("igemm ") for r in routes) and any("nbuf3" in r for r in routes)
    assert {r.split()[1] for r in routes if r.startswith("igemm ")} >= {"128x128", "128x64", "128x32", "64x128", "64x64"}
    print("routes reached:", ", ".join(sorted(set(routes))))


@pytest.fixture(scope="module")
def bf16_engine():
    from sylph_amd.engine import Engine
    eng = Engine(None, dtype="bf16")
    eng.profile_enable(True)
    return eng


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_conv_route_pinned_to_bf16_ulps(case, bf16_engine):
    B, cin, h, w, cout, k, s, relu, use_res, route = case
    x, wt, scale, shift, res = _operands(case, True)
    eng = bf16_engine
    eng.conv_routes(), eng.profile_read()  # nothing left over from an earlier case
    y = eng.conv2d(x, wt, scale, shift, s, k // 2, relu, res).cpu()
    routes, kernels = eng.conv_routes(), sorted(eng.profile_read()["kernels"])
    want = bf16_rne(conv_epilogue_f64(x, wt, scale, shift, s, k // 2, relu, res))
    assert_ulps(y, want, f"{_case_id(case)} on {routes}")
    if _overrides():
        pytest.skip(f"routing overrides set ({', '.join(_overrides())}): the numbers are checked, the route is not the default one")
    assert routes == [route], f"{_case_id(case)}: expected route {route!r}, ran {routes}"
    assert kernels == [KERNEL_OF.get(route.split()[0], "conv_igemm_kernel")], (route, kernels)


# one case per geometry class: 1x1, 1x1 strided, 3x3, 3x3 strided, residual, Cout not a tile multiple
F32_CASES = [
    (2, 256, 20, 24, 128, 1, 1, True, True, None),
    (2, 256, 18, 22, 128, 1, 2, True, False, None),
    (1, 512, 15, 19, 256, 3, 1, False, False, None),
    (2, 128, 21, 13, 80, 3, 2, True, False, None),
    (1, 64, 17, 23, 6, 3, 1, False, True, None),
]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f32", "f32s"])
@pytest.mark.parametrize("case", F32_CASES, ids=[_case_id(c) for c in F32_CASES])
def test_conv_fp32_modes_within_derived_bound(case, mode):
    """fp32 storage modes against float64, per element, with the bound of the module docstring."""
    from sylph_amd.engine import Engine
    B, cin, h, w, cout, k, s, relu, use_res, _ = case
    x, wt, scale, shift, res = _operands(case, False)
    y = Engine(None, dtype=mode).conv2d(x, wt, scale, shift, s, k // 2, relu, res).cpu().double()
    want = conv_epilogue_f64(x, wt, scale, shift, s, k // 2, relu, res)
    S = conv_epilogue_f64(x.abs(), wt.abs(), scale.abs(), shift.abs(), s, k // 2, False, res.abs() if res is not None else None)
    u, K = 2.0 ** -24, cin * k * k
    bound = 8.0 * (K + 3) ** 0.5 * u * S + (2.0 ** -16 * S if mode == "f32s" else 0.0)
    ratio = float(((y - want).abs() / bound).max())
    print(f"{mode} {_case_id(case)}: worst error {ratio:.3f} of the bound")
    assert ratio <= 1.0, f"{mode} {_case_id(case)}: error {ratio:.3f} x the derived bound"
