"""The last res2 block computed only where res3 reads it (bottleneck64_kernel<3, 1, 2, false, true>, SYLPH_BK_STRIDED_TAIL).

With STRIDE_IN_1X1 the first res3 block takes every other row and column of res2, and res2 is no FPN input: the last identity
block of res2 writes a compact (H/2, W/2) tensor holding its output at the even positions, and res3.0 runs its own launches on
that tensor with stride 1.  The strided build keeps the dense build's MFMA shapes, accumulation orders and rounding points, so
every check here is BIT identity -- against the dense kernel, against the graph with the knob off, and for the res2 parity tap,
which runs the dense launch on demand."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

KERNEL = "bottleneck64_kernel"


def _block(seed, B, H, W):
    from oracle import bf16 as OB16
    g = torch.Generator().manual_seed(seed)
    x = OB16.r(F.relu(torch.randn(B, 256, H, W, generator=g)))

    def conv(co, ci, k):
        return torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5
    ws = [conv(64, 256, 1), conv(64, 64, 3), conv(256, 64, 1)]
    scales = [0.5 + torch.rand(w.shape[0], generator=g) for w in ws]
    shifts = [0.2 * torch.randn(w.shape[0], generator=g) for w in ws]
    return x, ws, scales, shifts


def _engine(cfg=None):
    from sylph_amd.engine import Engine
    return Engine(cfg, dtype="bf16")


# (8, 8): one partial tile; (10, 16): exactly one 5 x 8 tile; (12, 18): ragged in both directions; (16, 16): fewer tiles than the
# 8-way XCD walk; B = 3: the per-image base.  (200, 336): the production map, 420 tiles of one image.  The tile is chosen per map
# (fewest tiles, bottleneck64_even_patch), which fits these small maps exactly where it can: (26, 38) -- 13 x 19 outputs, 7 x 5 tiles --
# and (22, 34) -- 11 x 17 outputs, 6 x 6 tiles -- have prime output sizes, so their last tile row and column are partial whatever
# the tile.
@pytest.mark.parametrize("B,H,W", [(3, 8, 8), (3, 10, 16), (3, 12, 18), (3, 16, 16), (3, 26, 38), (2, 22, 34), (1, 200, 336)])
def test_strided_kernel_equals_dense_kernel_at_even_positions(B, H, W):
    x, ws, scales, shifts = _block(100 * H + W, B, H, W)
    eng = _engine()
    eng.profile_enable(True)
    eng.profile_read()
    even = eng.bottleneck_even(x, ws, scales, shifts)
    k_even = eng.profile_read()["kernels"]
    dense = eng.bottleneck(x, ws, scales, shifts, 1)
    k_dense = eng.profile_read()["kernels"]
    eng.profile_enable(False)
    assert even.shape == (B, 256, H // 2, W // 2) and torch.isfinite(even).all()
    assert float(even.abs().max()) > 0.0
    want = dense[..., ::2, ::2]
    bad = int((even != want).sum())
    print(f"({B}, {H}, {W}): {bad} of {want.numel()} values differ")
    assert torch.equal(even, want), f"({B}, {H}, {W}): {bad} of {want.numel()} values differ from the dense kernel's"
    for what, k in (("bottleneck_even", k_even), ("bottleneck", k_dense)):
        assert list(k) == [KERNEL] and k[KERNEL]["launches"] == 1, f"{what}: {k}"
    # conv1 everywhere, conv2 / conv3 on a quarter of the positions
    assert k_even[KERNEL]["flops"] == pytest.approx(2.0 * B * (H * W * 256 * 64 + (H // 2) * (W // 2) * (64 * 576 + 64 * 256)))


@pytest.mark.parametrize("H,W", [(9, 16), (10, 15), (7, 7)])
def test_strided_kernel_refuses_odd_maps(H, W):
    x, ws, scales, shifts = _block(3, 1, H, W)
    eng = _engine()
    with pytest.raises(RuntimeError, match="even"):
        eng.bottleneck_even(x, ws, scales, shifts)
    # the context is still good
    y = eng.bottleneck(x, ws, scales, shifts, 1)
    assert torch.isfinite(y).all()


def test_strided_kernel_refuses_other_block_shapes():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 512, 8, 8, generator=g)
    ws = [torch.randn(128, 512, 1, 1, generator=g), torch.randn(128, 128, 3, 3, generator=g), torch.randn(512, 128, 1, 1, generator=g)]
    scales = [torch.ones(w.shape[0]) for w in ws]
    shifts = [torch.zeros(w.shape[0]) for w in ws]
    with pytest.raises(RuntimeError, match="C 256, mid 64"):
        _engine().bottleneck_even(x, ws, scales, shifts)


# One child process per (shape, knob): the knob is read once per process.  It runs the step twice -- plain, then with the res2 tap
# called around the other taps -- and saves everything the checks below compare.
_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
from sylph_amd import synthetic as W
from test_hip_parity import _engine, _cfg
B, H, Wd = int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6])
eng = _engine("bf16", _cfg())
eng.load_state_dict(W.synthetic_state_dict(0, depth=50))
imgs = W.synthetic_images(B, H, Wd, seed=11)
codes = W.synthetic_codes(5, seed=4, scale=3.0)
out = {}
def np_(t): return t.float().cpu().numpy()
def dets(tag):
    for i, d in enumerate(eng.decode()):
        for k, v in d.items():
            if torch.is_tensor(v): out[f"{tag}_det{i}_{k}"] = np_(v)
# plain step
eng.profile_enable(True); eng.profile_read()
eng.preprocess(imgs); eng.backbone()
out["flops"] = np.array(eng.profile_read()["kernels"]["bottleneck64_kernel"]["flops"])
eng.profile_enable(False)
for l, t in enumerate(eng.export_pyramid()): out[f"plain_p{l}"] = np_(t)
out["plain_res3"] = np_(eng.export_stage(3))
eng.head(codes["cls_conv"], codes["cls_bias"]); dets("plain")
# the same step with the res2 tap in between
eng.preprocess(imgs); eng.backbone()
out["tap_res3_before"] = np_(eng.export_stage(3))
for l, t in enumerate(eng.export_pyramid()): out[f"tapbefore_p{l}"] = np_(t)
eng.profile_enable(True); eng.profile_read()
out["res2"] = np_(eng.export_stage(2))
k = eng.profile_read()["kernels"]
out["tap_launches"] = np.array(k.get("bottleneck64_kernel", {"launches": 0})["launches"])
eng.profile_enable(False)
out["tap_res3_after"] = np_(eng.export_stage(3))
out["res4"] = np_(eng.export_stage(4))
out["res2_again"] = np_(eng.export_stage(2))
for l, t in enumerate(eng.export_pyramid()): out[f"tapafter_p{l}"] = np_(t)
eng.head(codes["cls_conv"], codes["cls_bias"]); dets("tap")
np.savez(sys.argv[3], **out)
"""

SHAPES = [(1, 200, 232), (3, 72, 328), (2, 40, 56)]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{(B, H, W): {"on": arrays, "off": arrays}}, computed once for the module."""
    td = tmp_path_factory.mktemp("strided_tail")
    outs = {}
    for B, H, W in SHAPES:
        outs[(B, H, W)] = {}
        for name, knob in (("on", "1"), ("off", "0")):
            path = str(td / f"{B}_{H}_{W}_{name}.npz")
            r = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(ROOT, "sylph-few-shot-detection_amd"), os.path.join(ROOT, "tests"), path,
                                str(B), str(H), str(W)], env=dict(os.environ, SYLPH_BK_STRIDED_TAIL=knob), cwd=ROOT, capture_output=True,
                               text=True, timeout=600)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            z = np.load(path)
            outs[(B, H, W)][name] = {k: z[k] for k in z.files}
    return outs


@pytest.mark.parametrize("shape", SHAPES)
def test_backbone_with_strided_tail_is_bit_identical(runs, shape):
    """Pyramid and res3 with the knob on and off: the same bits on every level, on maps ragged in both directions."""
    on, off = runs[shape]["on"], runs[shape]["off"]
    if "SYLPH_FUSE_BOTTLENECK" not in os.environ:  # the strided launch ran: conv2 / conv3 of one of the two launches on a quarter
        assert float(on["flops"]) < float(off["flops"]), (float(on["flops"]), float(off["flops"]))
    keys = ["plain_res3"] + [f"plain_p{l}" for l in range(5)]
    for k in keys:
        assert on[k].shape == off[k].shape and np.isfinite(on[k]).all()
        assert np.array_equal(on[k], off[k]), f"{shape} {k}: {int((on[k] != off[k]).sum())} values differ, max {np.abs(on[k] - off[k]).max()}"
    dk = sorted(k for k in off if k.startswith("plain_det"))
    assert dk and dk == sorted(k for k in on if k.startswith("plain_det"))
    for k in dk:
        assert np.array_equal(on[k], off[k]), f"{shape} {k}"


def test_res2_tap_is_exact_and_disturbs_nothing(runs):
    """With the knob on res2 exists at the even positions only: the tap runs the dense launch on demand.  It returns the dense
    graph's res2 bit for bit, any number of times, and leaves res3, res4, the pyramid and the detections as they were."""
    shape = SHAPES[2]
    on, off = runs[shape]["on"], runs[shape]["off"]
    assert on["res2"].shape == off["res2"].shape and on["res2"].shape[1] == 256
    assert np.array_equal(on["res2"], off["res2"]), f"{int((on['res2'] != off['res2']).sum())} res2 values differ"
    assert np.array_equal(on["res2_again"], off["res2"])
    if "SYLPH_FUSE_BOTTLENECK" not in os.environ:
        assert int(on["tap_launches"]) == 1 and int(off["tap_launches"]) == 0  # the on-demand dense launch; the dense graph has none to run
    for r in (on, off):
        assert np.array_equal(r["tap_res3_before"], r["tap_res3_after"]) and np.array_equal(r["tap_res3_after"], r["plain_res3"])
        for l in range(5):
            assert np.array_equal(r[f"tapbefore_p{l}"], r[f"tapafter_p{l}"]) and np.array_equal(r[f"tapafter_p{l}"], r[f"plain_p{l}"]), l
        dk = sorted(k for k in r if k.startswith("plain_det"))
        assert dk
        for k in dk:
            assert np.array_equal(r[k], r["tap" + k[len("plain"):]]), k
    assert np.array_equal(on["res4"], off["res4"])
