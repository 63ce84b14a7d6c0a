"""Golden classification targets from the REFERENCE's own FCOSOutputs (imported through tests/golden/ref_shim.py, with the helpers of
gen_goldens.py).  Run in the build container:

    python tests/golden/gen_finetune_golden.py

Writes tests/golden/g12_fcos_targets.npz (data only): for every case the boxes, classes and image indices of a two-image batch padded to
128 x 160 (levels of 640 / 160 / 40 / 12 / 4 locations over the two images) and the `labels` of MetaFCOS.fcos_outputs._get_ground_truth per level, (2, h w);
`back_ground_id` is the reference's.

  a_on / a_off   image 0: a box covering the whole image, a box smaller than one stride-8 cell, two overlapping boxes of equal area with
                 different classes; image 1: no box.  Centre sampling on (POS_RADIUS 1.5) / off
  b_on / d_on    one box per image whose largest regression target sits, at a location inside its sample region, exactly on 64 (b: image 0
                 on P3, image 1 on P4) resp. on 128 (d: image 0 on P4, image 1 on P5): `<=` and `>=` of is_cared_in_the_level
  c_on           image 1 starts with a box whose centre-x is 0: get_sample_region returns an empty region for the whole image
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import gen_goldens as G  # noqa: E402  (installs ref_shim, puts the repo and the package on sys.path)

H, W = 128, 160
SIZES = [(128, 153), (123, 160)]

CASES = {
    "a": ([[0, 0, 160, 128, 0, 0], [33, 41, 38, 46, 1, 0], [20, 20, 80, 60, 2, 0], [40, 30, 100, 70, 3, 0]], True),
    "b": ([[4, 40, 124, 100, 0, 0], [8, 30, 120, 98, 1, 1]], True),
    "d": ([[8, 40, 220, 100, 3, 0], [16, 8, 200, 120, 2, 1]], True),
    "c": ([[30, 30, 90, 90, 0, 0], [10, 50, 150, 120, 4, 0], [-20, 10, 20, 50, 1, 1], [30, 30, 90, 90, 2, 1]], True),
}


def targets(cfg, rows):
    from sylph.modeling.meta_fcos.fcos import MetaFCOS
    from ref_shim import Boxes, Instances, ShapeSpec
    shapes = {f"p{l}": ShapeSpec(channels=256, stride=2 ** l) for l in range(3, 8)}
    model = MetaFCOS(cfg, shapes).eval()
    feats = [torch.zeros(2, 256, h, w) for h, w in ((16, 20), (8, 10), (4, 5), (2, 3), (1, 2))]
    locations = model.compute_locations(feats)
    rows = torch.tensor(rows, dtype=torch.float32).reshape(-1, 6)
    insts = []
    for i in range(2):
        m = rows[:, 5] == i
        it = Instances(SIZES[i])
        it.gt_boxes = Boxes(rows[m, :4])
        it.gt_classes = rows[m, 4].long()
        insts.append(it)
    with torch.no_grad():
        tt = model.fcos_outputs._get_ground_truth(locations, insts)
    return [t.reshape(2, -1).numpy() for t in tt["labels"]], int(model.fcos_outputs.back_ground_id)


if __name__ == "__main__":
    out = {}
    for name, (rows, _) in CASES.items():
        for tag, cs in (("on", True), ("off", False)):
            if tag == "off" and name != "a":
                continue
            cfg = G.make_cfg()
            cfg.MODEL.FCOS.CENTER_SAMPLE = cs
            cfg.MODEL.FCOS.POS_RADIUS = 1.5
            labels, bg = targets(cfg, rows)
            r = np.array(rows, np.float32)
            out[f"{name}_{tag}_boxes"] = r[:, :4]
            out[f"{name}_{tag}_classes"] = r[:, 4].astype(np.int64)
            out[f"{name}_{tag}_image"] = r[:, 5].astype(np.int64)
            out[f"{name}_{tag}_center_sample"] = np.array(cs)
            for l, t in enumerate(labels):
                out[f"{name}_{tag}_labels{l}"] = t.astype(np.int64)
            out["back_ground_id"] = np.array(bg)
            print(name, tag, "positives per level", [int((t != bg).sum()) for t in labels], "background id", bg)
    out["pos_radius"] = np.array(1.5)
    out["padded_hw"] = np.array([H, W])
    path = os.path.join(HERE, "g12_fcos_targets.npz")
    np.savez_compressed(path, **out)
    print("done", os.path.getsize(path), "bytes")
