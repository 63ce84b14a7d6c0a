"""The res3 block-pair route inside the R-50 backbone (SYLPH_BLOCK_PAIR; build_backbone, csrc/api_backbone.hip): block i's conv3 launch
also computes block i + 1's conv1 (conv_spw_kernel_pair), for the pairs 1 -> 2 and 2 -> 3 of res3.

With the knob at 2 the route runs wherever the shapes allow; its y is what conv3 gives, its t1 may differ from the separate conv1 by one
bf16 ulp (another kernel sums the same products), so pyramid and res3 agree with the knob-off graph under assert_chain at its defaults.
With the knob unset the launch-size threshold keeps these small shapes off the route, and the graph is the knob-off graph bit for bit.

The knob is read once per process: one child per (shape, knob), run once for the module."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from bf16_ulps import assert_chain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

# res3 maps of 20 x 28 = 560 rows (8 full tiles of 64 and a ragged one per image) and 12 x 44 = 528 (8 and a quarter)
SHAPES = [(2, 160, 224), (1, 96, 352)]
PAIR_ROUTE = "spw_pair 64x512+128"

_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
from sylph_amd import synthetic as W
from test_hip_parity import _engine, _cfg
B, H, Wd = int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6])
eng = _engine("bf16", _cfg())
eng.load_state_dict(W.synthetic_state_dict(0, depth=50))
imgs = W.synthetic_images(B, H, Wd, seed=11)
out = {}
eng.profile_enable(True); eng.profile_read(); eng.conv_routes()
eng.preprocess(imgs); eng.backbone()
routes = eng.conv_routes()
kern = eng.profile_read()["kernels"]
eng.profile_enable(False)
out["n_pair_routes"] = np.array(sum(r == sys.argv[7] for r in routes))
out["n_pair_launches"] = np.array(kern.get("conv_spw_kernel_pair", {"launches": 0})["launches"])
for l, t in enumerate(eng.export_pyramid()): out[f"p{l}"] = t.float().cpu().numpy()
out["res3"] = eng.export_stage(3).float().cpu().numpy()
np.savez(sys.argv[3], **out)
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{(B, H, W): {"2" | "0" | "unset": arrays}}"""
    td = tmp_path_factory.mktemp("res3_pair_backbone")
    outs = {}
    for B, H, W in SHAPES:
        outs[(B, H, W)] = {}
        for knob in ("2", "0", "unset"):
            env = {k: v for k, v in os.environ.items() if k != "SYLPH_BLOCK_PAIR"}
            if knob != "unset":
                env["SYLPH_BLOCK_PAIR"] = knob
            path = str(td / f"{B}_{H}_{W}_{knob}.npz")
            r = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(ROOT, "sylph-few-shot-detection_amd"), os.path.join(ROOT, "tests"), path,
                                str(B), str(H), str(W), PAIR_ROUTE], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            z = np.load(path)
            outs[(B, H, W)][knob] = {k: z[k] for k in z.files}
    return outs


@pytest.mark.parametrize("shape", SHAPES)
def test_pair_route_runs_only_where_asked(runs, shape):
    r = runs[shape]
    assert int(r["2"]["n_pair_routes"]) == 2 and int(r["2"]["n_pair_launches"]) == 2, (r["2"]["n_pair_routes"], r["2"]["n_pair_launches"])
    for knob in ("0", "unset"):  # unset: these launches are below the size threshold
        assert int(r[knob]["n_pair_routes"]) == 0 and int(r[knob]["n_pair_launches"]) == 0, knob


@pytest.mark.parametrize("shape", SHAPES)
def test_backbone_with_pair_route_agrees_with_the_chain(runs, shape):
    on, off = runs[shape]["2"], runs[shape]["0"]
    for k in ["res3"] + [f"p{l}" for l in range(5)]:
        assert on[k].shape == off[k].shape and np.isfinite(on[k]).all()
        assert_chain(torch.from_numpy(on[k]), torch.from_numpy(off[k]), f"{shape} {k}")


@pytest.mark.parametrize("shape", SHAPES)
def test_default_knob_is_the_chain_at_small_shapes(runs, shape):
    unset, off = runs[shape]["unset"], runs[shape]["0"]
    for k in ["res3"] + [f"p{l}" for l in range(5)]:
        assert np.array_equal(unset[k], off[k]), f"{shape} {k}: {int((unset[k] != off[k]).sum())} values differ"
