"""The outputs of codegen, codegen_classes and roi_align on small one-box-per-image batches, as numpy arrays:
tests/golden/gen_parent_support_golden.py records them in g12_parent_support.npz, tests/test_support_rois_gpu.py recomputes them with
the current build and compares bit for bit.  TEST INFRASTRUCTURE; needs a GPU.

Cases, on 64 x 96 pyramids (helpers of tests/test_support_bf16_pinned_gpu.py): several classes whose rows start at non-zero offsets
(12 images, 3 shots), one-shot classes (12 images, 1 shot), one class per call (5 images), and in bf16 two classes at the 64-shot cap
(128 images: a full wave of softmax terms, the second class's rows starting at 64); ROIAlign alone on the boxes that straddle a
border, lie outside the image or are thin."""
from typing import Dict

import torch

H, W = 64, 96
KINDS = ("codegen", "weighted", "roienc")
DTYPES = ("bf16", "f32", "f32s")


def outputs_support() -> Dict[str, "np.ndarray"]:
    from test_support_bf16_pinned_gpu import _box_kinds, _box_sets, _engine, _pyramid
    out = {}

    def record(eng, key, kind, codes, n_codes):
        out[f"{key}_codes"] = codes.cpu().numpy()
        if kind == "weighted":
            out[f"{key}_wnorm"] = eng.codegen_weight_norm(n_codes).cpu().numpy()
        if kind == "roienc":
            out[f"{key}_cls_tokens"] = eng.export_support("cls_tokens").cpu().numpy()

    for kind in KINDS:
        for dtype in DTYPES:
            eng = _engine(kind, dtype=dtype, taps=False)
            eng.import_pyramid(_pyramid(12, H, W, seed=112), (H, W))
            boxes = _box_sets(12, H, W, seed=612)[0]
            for shots in (3, 1):
                record(eng, f"{kind}_{dtype}_b12_s{shots}", kind, eng.codegen_classes(boxes, shots), 12 // shots)
            eng.import_pyramid(_pyramid(5, H, W, seed=105), (H, W))
            record(eng, f"{kind}_{dtype}_b5_one", kind, eng.codegen(_box_sets(5, H, W, seed=605)[0])[None], 1)
            if dtype == "bf16" and kind != "roienc":
                eng.import_pyramid(_pyramid(128, H, W, seed=228), (H, W))
                record(eng, f"{kind}_{dtype}_b128_s64", kind, eng.codegen_classes(_box_sets(128, H, W, seed=728)[0], 64), 2)
            if kind == "codegen" and dtype != "f32s":
                eng.import_pyramid(_pyramid(4, H, W, seed=104), (H, W))
                edges = _box_kinds(H, W)[5:13]  # straddling left / top / right / bottom | outside x 2, thin x 2
                for j in range(2):
                    out[f"roi_align_{dtype}_{j}"] = eng.roi_align(edges[4 * j:4 * j + 4]).cpu().numpy()
            eng.close()
    return out
