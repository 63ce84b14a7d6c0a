"""Pins sylph_codegen / sylph_codegen_classes / sylph_roi_align to the bits of the commit whose message begins "Head: one GroupNorm
stream core": run on an MI355X with the library built from that commit (it exports the same C ABI, so the host code of the current
tree drives it):

    SYLPH_LIB_PATH=<that build>/libsylph_hip.so python tests/golden/gen_parent_support_golden.py [out.npz]

Writes tests/golden/g12_parent_support.npz: support_parent_ref.outputs_support -- raw codes of the plain generator, the weighted one
(with cls_weight_norm) and the ROIEncoder (with its class tokens) in bf16, fp32 and split-bf16, and ROIAlign on edge boxes.
tests/test_support_rois_gpu.py asserts np.array_equal against it."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "sylph-few-shot-detection_amd"), os.path.dirname(HERE)):
    sys.path.insert(0, p)

from support_parent_ref import outputs_support  # noqa: E402

if __name__ == "__main__":
    if not os.environ.get("SYLPH_LIB_PATH"):
        raise SystemExit("set SYLPH_LIB_PATH to the library of the pinned commit (see the docstring)")
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g12_parent_support.npz")
    out = outputs_support()
    np.savez_compressed(path, **out)
    print("done", len(out), "arrays", os.path.getsize(path), "bytes")
