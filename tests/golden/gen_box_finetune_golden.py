"""Golden regression targets and box losses from the REFERENCE's own FCOSOutputs (imported through tests/golden/ref_shim.py, with the
helpers of gen_goldens.py).  Run in the build container:

    python tests/golden/gen_box_finetune_golden.py

Writes tests/golden/g13_box_losses.npz (data only).  For the cases a_on / a_off / b_on / c_on / d_on of gen_finetune_golden.py (the
two-image batch padded to 128 x 160), with FREEZE_BBOX_BRANCH False so that box_branch_loss_on holds:

  {case}_boxes / _classes / _image / _center_sample      the annotations, as in g12
  {case}_labels{l}, {case}_reg_targets{l}                 `labels` (2, h w) and `reg_targets` (2, h w, 4) of _get_ground_truth per level,
                                                          the latter divided by the stride (fcos_outputs.py:185-189)
  {case}_pos_reg_pred / _pos_ctr_pred / _pos_iou_pred     fixed random predictions at the positives, in fcos_losses' order (level-major), and
  {case}_pos_reg_targets / _pos_level                     their targets and levels
  {case}_{quality}_{mask}_loc / _ctr / _iou               the values of loss_fcos_loc / loss_fcos_ctr / loss_fcos_iou (float32; nan where
                                                          fcos_losses does not return the loss) for quality in ctrness / iou / both, mask 0 / 1
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import gen_goldens as G  # noqa: E402  (installs ref_shim, puts the repo and the package on sys.path)
from gen_finetune_golden import CASES, SIZES  # noqa: E402

QUALITIES = {"ctrness": ["ctrness"], "iou": ["iou"], "both": ["ctrness", "iou"]}
LEVELS = ((16, 20), (8, 10), (4, 5), (2, 3), (1, 2))


def model_for(center_sample, quality, iou_mask):
    from sylph.modeling.meta_fcos.fcos import MetaFCOS
    from ref_shim import ShapeSpec
    cfg = G.make_cfg()
    cfg.MODEL.FCOS.CENTER_SAMPLE = center_sample
    cfg.MODEL.FCOS.POS_RADIUS = 1.5
    cfg.MODEL.FCOS.BOX_QUALITY = quality
    cfg.MODEL.FCOS.IOU_MASK = bool(iou_mask)
    cfg.MODEL.PROPOSAL_GENERATOR.FREEZE_BBOX_BRANCH = False
    shapes = {f"p{l}": ShapeSpec(channels=256, stride=2 ** l) for l in range(3, 8)}
    return MetaFCOS(cfg, shapes).eval()


def ground_truth(model, rows):
    from ref_shim import Boxes, Instances
    feats = [torch.zeros(2, 256, h, w) for h, w in LEVELS]
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
        return model.fcos_outputs._get_ground_truth(locations, insts)


if __name__ == "__main__":
    from ref_shim import Instances
    import sylph.modeling.meta_fcos.fcos_outputs as FO
    FO.reduce_sum = lambda t: t  # one rank (the shim leaves the comm helpers inert)
    FO.get_world_size = lambda: 1
    FO.sigmoid_focal_loss_jit = lambda x, t, **kw: x.sum() * 0  # loss_fcos_cls is not part of this golden (g12 / finetune_ref pin it)
    out = {}
    for name, (rows, _) in CASES.items():
        for tag, cs in (("on", True), ("off", False)):
            if tag == "off" and name != "a":
                continue
            case = f"{name}_{tag}"
            tt = ground_truth(model_for(cs, ["ctrness"], False), rows)
            r = np.array(rows, np.float32)
            out[f"{case}_boxes"] = r[:, :4]
            out[f"{case}_classes"] = r[:, 4].astype(np.int64)
            out[f"{case}_image"] = r[:, 5].astype(np.int64)
            out[f"{case}_center_sample"] = np.array(cs)
            for l, (lab, reg) in enumerate(zip(tt["labels"], tt["reg_targets"])):
                out[f"{case}_labels{l}"] = lab.reshape(2, -1).numpy().astype(np.int64)
                out[f"{case}_reg_targets{l}"] = reg.reshape(2, -1, 4).numpy().astype(np.float32)
            # fcos_losses' instances: every location, level-major (fcos_outputs.py:351-420 flattens the per-level tensors in that order)
            labels = torch.cat([x.reshape(-1) for x in tt["labels"]])
            reg_targets = torch.cat([x.reshape(-1, 4) for x in tt["reg_targets"]])
            level = torch.cat([torch.full((x.numel(),), l) for l, x in enumerate(tt["labels"])])
            n = labels.numel()
            g = torch.Generator().manual_seed(131 + len(out))
            reg_pred = torch.rand(n, 4, generator=g) * 6.0 + 0.05
            ctr_pred = torch.randn(n, generator=g) * 2.0
            iou_pred = torch.randn(n, generator=g) * 2.0
            for qn, q in QUALITIES.items():
                for mask in (0, 1):
                    model = model_for(cs, q, mask)
                    fo = model.fcos_outputs
                    it = Instances((0, 0))
                    it.labels = labels.clone()
                    it.logits_pred = torch.zeros(n, fo.num_classes)
                    it.reg_pred = reg_pred.clone()
                    it.reg_targets = reg_targets.clone()
                    it.ctrness_pred = ctr_pred.clone()
                    it.iou_pred = iou_pred.clone()
                    with torch.no_grad():
                        extras, losses = fo.fcos_losses(it)
                    for key, short in (("loss_fcos_loc", "loc"), ("loss_fcos_ctr", "ctr"), ("loss_fcos_iou", "iou")):
                        out[f"{case}_{qn}_{mask}_{short}"] = np.array(float(losses[key]) if key in losses else np.nan, np.float32)
            pos = labels != model.fcos_outputs.back_ground_id
            out[f"{case}_pos_reg_pred"] = reg_pred[pos].numpy()
            out[f"{case}_pos_ctr_pred"] = ctr_pred[pos].numpy()
            out[f"{case}_pos_iou_pred"] = iou_pred[pos].numpy()
            out[f"{case}_pos_reg_targets"] = reg_targets[pos].numpy()
            out[f"{case}_pos_level"] = level[pos].numpy().astype(np.int64)
            out["back_ground_id"] = np.array(int(model.fcos_outputs.back_ground_id))
            print(case, "positives", int(pos.sum()), {k: float(v) for k, v in out.items() if k.startswith(f"{case}_both_1_")})
    out["pos_radius"] = np.array(1.5)
    out["padded_hw"] = np.array([128, 160])
    path = os.path.join(HERE, "g13_box_losses.npz")
    np.savez_compressed(path, **out)
    print("done", os.path.getsize(path), "bytes")
