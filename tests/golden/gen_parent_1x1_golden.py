"""Pins what the 1x1-code path computed BEFORE class codes got a spatial size: run on an MI355X with the library built from the commit
that precedes `sylph_config::cg_code_ksize` (the host code of the current tree drives it; a library without the field leaves it 0 and
the engine runs 1x1 codes):

    SYLPH_LIB_PATH=<that build>/libsylph_hip.so python tests/golden/gen_parent_1x1_golden.py [out.npz]

Writes tests/golden/g11_parent_1x1.npz: spatial_codes_ref.outputs_1x1 -- bf16 head outputs and detections on g1, support codes (bf16,
fp32; class and ROI-list form) and their normalisation on g3.  tests/test_spatial_codes_gpu.py asserts torch.equal against it."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "sylph-few-shot-detection_amd"), os.path.dirname(HERE)):
    sys.path.insert(0, p)

from spatial_codes_ref import outputs_1x1  # noqa: E402

if __name__ == "__main__":
    if not os.environ.get("SYLPH_LIB_PATH"):
        raise SystemExit("set SYLPH_LIB_PATH to the library of the commit before cg_code_ksize")
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g11_parent_1x1.npz")
    out = outputs_1x1(HERE)
    np.savez_compressed(path, **out)
    print("done", len(out), "arrays", os.path.getsize(path), "bytes")
