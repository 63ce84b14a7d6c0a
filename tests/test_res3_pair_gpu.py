"""The res3 block-pair kernel alone (conv_spw_kernel_pair, csrc/conv_spw_pair.hip; Engine.res3_pair):

    y  = relu(bn3(w3 t2) + x)      conv3 + residual of a res3 identity block     (B, 512, H, W)
    t1 = relu(bn1(w1 y))           conv1 of the next block, from the bf16 y      (B, 128, H, W)

  * y is BIT-identical to conv_spw_kernel<128, 1, true> on the same operands (Engine.conv2d with SYLPH_CONV_SPW=2, route asserted): the
    pair kernel keeps that kernel's MFMAs, k order, epilogue and rounding point.
  * y against float64: conv_epilogue_f64 + ONE bf16 RNE rounding, at the single-conv bound of tests/test_conv_routes_gpu.py -- worst
    element <= 1 bf16 ulp (floor 1e-3 of the tensor maximum), <= 1 % of elements not identical.
  * t1 against the float64 reference computed FROM THE KERNEL'S OWN bf16 y, at the same bound: the second GEMM sums exact bf16 products
    in fp32 and rounds once, like any single conv.

Channels are fixed (512 / 128); a tile is 64 positions of one image, all channels wide, and the grid is min(tiles, CUs) persistent blocks.
Shapes: B = 2 of 13 x 21 -- 273 rows per image: four full tiles and a ragged one in each image, no tile straddling two images; B = 1 of
8 x 8 -- one tile, a single block; B = 3 of 50 x 84 -- 66 tiles per image, 198 in all (no multiple of 8), the last of each image ragged;
B = 110 of 13 x 21 -- 550 tiles on at most 256 blocks: a block walks a first, a middle and a last tile, so the A buffer, the double y
buffer and the t1 staging are reused across tiles (the first three cases run one tile per block on a 256-CU part).  One case is run
twice on the same engine: identical bits (stale LDS or buffer state across launches).

The comparison kernel is forced by an environment knob that is read once per process, so the GPU work of the module runs in ONE child
process, once; the float64 references are computed here."""
import os
import subprocess
import sys

import pytest
import torch

from bf16_ulps import assert_ulps, bf16_rne, conv_epilogue_f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

# B, H, W
SHAPES = [(2, 13, 21), (1, 8, 8), (3, 50, 84), (110, 13, 21)]
TWICE = (2, 13, 21)

_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from sylph_amd.engine import Engine
shapes = [tuple(int(v) for v in s.split("x")) for s in sys.argv[3].split(",")]
twice = tuple(int(v) for v in sys.argv[4].split("x"))
eng = Engine(None, dtype="bf16")
out = {}
for (B, H, W) in shapes:
    g = torch.Generator().manual_seed(1000 * B + 10 * H + W)
    r = lambda t: t.bfloat16().float()
    t2 = r(torch.relu(torch.randn(B, 128, H, W, generator=g)))
    x = r(torch.relu(torch.randn(B, 512, H, W, generator=g)))
    w3 = r(torch.randn(512, 128, 1, 1, generator=g) * (2.0 / 128) ** 0.5)
    w1 = r(torch.randn(128, 512, 1, 1, generator=g) * (2.0 / 512) ** 0.5)
    s3, s1 = 0.5 + torch.rand(512, generator=g), 0.5 + torch.rand(128, generator=g)
    b3, b1 = 0.2 * torch.randn(512, generator=g), 0.2 * torch.randn(128, generator=g)
    eng.profile_enable(True); eng.profile_read(); eng.conv_routes()
    y_spw = eng.conv2d(t2, w3, s3, b3, relu=True, residual=x)
    routes_spw, k_spw = eng.conv_routes(), list(eng.profile_read()["kernels"])
    y, t1 = eng.res3_pair(t2, x, w3, s3, b3, w1, s1, b1)
    routes_pair, k_pair = eng.conv_routes(), list(eng.profile_read()["kernels"])
    eng.profile_enable(False)
    d = dict(t2=t2, x=x, w3=w3, w1=w1, s3=s3, b3=b3, s1=s1, b1=b1, y_spw=y_spw.cpu(), y=y.cpu(), t1=t1.cpu(),
             routes_spw=routes_spw, k_spw=k_spw, routes_pair=routes_pair, k_pair=k_pair)
    if (B, H, W) == twice:
        y2, t12 = eng.res3_pair(t2, x, w3, s3, b3, w1, s1, b1)
        d["y_again"], d["t1_again"] = y2.cpu(), t12.cpu()
    for k in ("t2", "x", "y_spw", "y", "t1", "y_again", "t1_again"):
        if k in d: d[k] = d[k].bfloat16()  # bf16 values: exact
    out[(B, H, W)] = d
torch.save(out, sys.argv[2])
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("res3_pair") / "runs.pt")
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(ROOT, "sylph-few-shot-detection_amd"), path,
                        ",".join("x".join(str(v) for v in s) for s in SHAPES), "x".join(str(v) for v in TWICE)],
                       env=dict(os.environ, SYLPH_CONV_SPW="2"), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = torch.load(path)
    os.remove(path)
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_that_ran(runs, shape):
    d = runs[shape]
    assert d["routes_spw"] == ["spw 128x256"] and d["k_spw"] == ["conv_spw_kernel"], (d["routes_spw"], d["k_spw"])
    assert d["routes_pair"] == ["spw_pair 64x512+128"] and d["k_pair"] == ["conv_spw_kernel_pair"], (d["routes_pair"], d["k_pair"])


@pytest.mark.parametrize("shape", SHAPES)
def test_y_is_bit_identical_to_conv_spw(runs, shape):
    d = runs[shape]
    B, H, W = shape
    assert d["y"].shape == (B, 512, H, W) and torch.isfinite(d["y"].float()).all() and float(d["y"].float().abs().max()) > 0.0
    bad = int((d["y"] != d["y_spw"]).sum())
    print(f"{shape}: {bad} of {d['y'].numel()} values differ from conv_spw's")
    assert torch.equal(d["y"], d["y_spw"]), f"{shape}: {bad} values differ from conv_spw's"


@pytest.mark.parametrize("shape", SHAPES)
def test_y_and_t1_against_float64(runs, shape):
    d = runs[shape]
    B, H, W = shape
    y_ref = bf16_rne(conv_epilogue_f64(d["t2"].float(), d["w3"], d["s3"], d["b3"], relu=True, res=d["x"].float()))
    assert_ulps(d["y"].float(), y_ref, f"{shape} y")
    assert d["t1"].shape == (B, 128, H, W) and float(d["t1"].float().abs().max()) > 0.0
    t1_ref = bf16_rne(conv_epilogue_f64(d["y"].float(), d["w1"], d["s1"], d["b1"], relu=True))  # from the kernel's own bf16 y
    assert_ulps(d["t1"].float(), t1_ref, f"{shape} t1")


def test_second_launch_on_the_same_engine_is_identical(runs):
    d = runs[TWICE]
    assert torch.equal(d["y"], d["y_again"]) and torch.equal(d["t1"], d["t1_again"])
