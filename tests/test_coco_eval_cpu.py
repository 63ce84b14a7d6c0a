"""COCO bbox evaluation, host side (no GPU): hand-derivable known answers that pin the numpy restatement tests/cocoeval_ref.py (the yardstick
of the GPU file), the C ABI's declarations, and DeviceCOCOEvaluator's host behaviour.  Every case keeps its IoUs clear of a threshold:
a hit is at IoU 1, 9/11, 2/3 or 0.62, a miss at 0 or 0.25."""
import math
import os
import re

import numpy as np
import pytest
import torch

import cocoeval_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# "precision 1" of the protocol is tp / (tp + np.spacing(1)): one step below 1 where tp = 1, exactly 1 from tp = 2 on; recalls are exact
ONE = pytest.approx(100.0, rel=1e-15)


def gt_of(anns, n_images=1, cats=(1,)):
    """anns: (image id, category id, [x, y, w, h], area or None -> w * h, iscrowd)"""
    return {"images": [{"id": i + 1} for i in range(n_images)], "categories": [{"id": c, "name": f"c{c}"} for c in cats],
            "annotations": [{"id": j + 1, "image_id": im, "category_id": c, "bbox": [float(v) for v in b],
                             "area": float(b[2] * b[3] if ar is None else ar), "iscrowd": cr} for j, (im, c, b, ar, cr) in enumerate(anns)]}


def det(im, c, box, score):
    return {"image_id": im, "category_id": c, "bbox": [float(v) for v in box], "score": score}


# ---- known answers -------------------------------------------------------------------------------------------------------------------
def test_perfect_detections_give_one_everywhere():
    boxes = [[5, 5, 20, 20], [5, 5, 60, 60], [5, 5, 150, 150]]  # small, medium, large: one per image, so AR@1 is 1 too
    gt = gt_of([(i + 1, 1, b, None, 0) for i, b in enumerate(boxes)], n_images=3)
    _, res = CR.results(gt, [det(i + 1, 1, b, 0.9) for i, b in enumerate(boxes)])
    for k in ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR@1", "AR@10", "AR@100", "ARs", "ARm", "ARl", "AP-c1"):
        assert res[k] == ONE, k


def test_higher_scored_miss_then_hit_at_iou_062():
    gt = gt_of([(1, 1, [0, 0, 100, 100], None, 0)])
    ev, res = CR.results(gt, [det(1, 1, [0, 0, 100, 62], 0.8), det(1, 1, [300, 300, 50, 50], 0.9)])
    assert CR.iou([0, 0, 100, 62], [0, 0, 100, 100], False) == 0.62
    assert res["AP50"] == 50.0  # precision 0, 1/2 -> 1/2 from the right at every recall threshold
    assert res["AP"] == pytest.approx(100 * 0.5 * 3 / 10, rel=1e-12)  # a hit at 0.5, 0.55 and 0.6 only
    assert np.all(ev["precision"][:3, :, 0, 0, 2] == 0.5) and np.all(ev["precision"][3:, :, 0, 0, 2] == 0.0)
    assert np.all(ev["recall"][:3, 0, 0, 2] == 1.0) and np.all(ev["recall"][3:, 0, 0, 2] == 0.0)
    assert ev["scores"][0, 0, 0, 0, 2] == 0.9 and np.all(ev["scores"][0, 1:, 0, 0, 2] == 0.8)  # recall 0 is reached by the miss


def test_detection_on_a_crowd_box_is_neither_tp_nor_fp():
    gt = gt_of([(1, 1, [0, 0, 50, 50], None, 0), (1, 1, [200, 200, 100, 100], None, 1)])
    dets = [det(1, 1, [210, 210, 20, 20], 0.9), det(1, 1, [0, 0, 50, 50], 0.5)]  # inside the crowd box first: IoU = its own area's share = 1
    m, ig, _, npig = CR.evaluate_pair(gt["annotations"], dets, CR.AREA_RNGS[0], 100)
    assert m.all() and ig[:, 0].all() and not ig[:, 1].any() and npig == 1
    assert CR.results(gt, dets)[1]["AP"] == ONE  # as a false positive it would halve the precision


def test_two_detections_match_the_same_crowd_box():
    gt = gt_of([(1, 1, [0, 0, 50, 50], None, 0), (1, 1, [200, 200, 100, 100], None, 1)])
    dets = [det(1, 1, [210, 210, 20, 20], 0.9), det(1, 1, [250, 250, 30, 30], 0.8), det(1, 1, [0, 0, 50, 50], 0.5)]
    m, ig, _, _ = CR.evaluate_pair(gt["annotations"], dets, CR.AREA_RNGS[0], 100)
    assert m.all() and ig[:, :2].all() and not ig[:, 2].any()
    assert CR.results(gt, dets)[1]["AP"] == ONE


def test_non_ignored_boxes_are_visited_first():
    # file order: a box whose area FIELD says large (ignored in "small"), then a small one; the detection fits the first exactly (IoU 1)
    # and the second at 9/11.  In the small range the second is visited first and the walk stops at the ignored one.
    gt = gt_of([(1, 1, [10, 10, 20, 20], 20000.0, 0), (1, 1, [10, 12, 20, 20], None, 0)])
    dets = [det(1, 1, [10, 10, 20, 20], 0.9)]
    assert CR.iou(dets[0]["bbox"], gt["annotations"][1]["bbox"], False) == pytest.approx(360 / 440)
    ev, res = CR.results(gt, dets)
    # file order would match the ignored box and leave the small one unmatched: 0.  The small box is hit at 9/11: thresholds 0.5 .. 0.8
    assert res["APs"] == pytest.approx(70.0, rel=1e-15) and np.all(ev["recall"][:7, 0, 1, 2] == 1.0) and np.all(ev["recall"][7:, 0, 1, 2] == 0.0)
    assert res["APl"] == ONE  # the area is the annotation's field, not w * h
    assert math.isnan(res["APm"])


def test_unmatched_detection_outside_the_range_is_ignored():
    gt = gt_of([(1, 1, [10, 10, 20, 20], None, 0)])
    dets = [det(1, 1, [300, 300, 200, 200], 0.9), det(1, 1, [10, 10, 20, 20], 0.8)]
    _, res = CR.results(gt, dets)
    assert res["APs"] == ONE and res["AP"] == 50.0


def test_category_with_only_crowd_ground_truth_reports_nan():
    gt = gt_of([(1, 1, [0, 0, 50, 50], None, 0), (1, 2, [0, 0, 80, 80], None, 1)], cats=(1, 2))
    ev, res = CR.results(gt, [det(1, 1, [0, 0, 50, 50], 0.9), det(1, 2, [0, 0, 80, 80], 0.9)])
    assert np.all(ev["precision"][:, :, 1] == -1) and np.all(ev["recall"][:, 1] == -1) and np.all(ev["scores"][:, :, 1] == -1)
    assert math.isnan(res["AP-c2"]) and res["AP-c1"] == ONE and res["AP"] == ONE


def test_last_of_two_equal_ious_is_taken():
    # the first detection overlaps both boxes at exactly 2/3 and takes the LATER one; the second reaches only the earlier one (2/3 vs 1/4)
    gt = gt_of([(1, 1, [8, 0, 10, 10], None, 0), (1, 1, [12, 0, 10, 10], None, 0)])
    dets = [det(1, 1, [10, 0, 10, 10], 0.9), det(1, 1, [6, 0, 10, 10], 0.8)]
    assert CR.iou(dets[0]["bbox"], gt["annotations"][0]["bbox"], False) == CR.iou(dets[0]["bbox"], gt["annotations"][1]["bbox"], False)
    _, res = CR.results(gt, dets)
    assert res["AP50"] == ONE and res["AR@100"] == pytest.approx(100 * 4 / 10)  # both hit at 0.5 .. 0.65


def test_max_dets_cut_per_image_and_category():
    boxes = [[0, 0, 40, 40], [100, 0, 40, 40], [200, 0, 40, 40]]
    gt = gt_of([(1, c, b, None, 0) for c in (1, 2) for b in boxes], cats=(1, 2))
    dets = [det(1, c, b, 0.9 - 0.1 * i) for c in (1, 2) for i, b in enumerate(boxes)]
    _, res = CR.results(gt, dets, max_dets=(1, 2, 3))
    assert res["AR@3"] == ONE  # six detections on the image, three per pair: a per-image cut would keep three of the six
    assert res["AR@1"] == pytest.approx(100 / 3) and res["AR@2"] == pytest.approx(200 / 3)


def test_equal_scores_order_by_image_then_rank():
    gt = gt_of([(2, 1, [0, 0, 50, 50], None, 0)], n_images=2)
    dets = [det(2, 1, [0, 0, 50, 50], 0.5), det(1, 1, [0, 0, 50, 50], 0.5)]  # the hit arrives first, but image 1 comes first
    _, res = CR.results(gt, dets)
    assert res["AP50"] == 50.0


def test_unknown_image_id_raises():
    gt = gt_of([(1, 1, [0, 0, 50, 50], None, 0)])
    with pytest.raises(ValueError, match="77"):
        CR.evaluate(gt, [det(77, 1, [0, 0, 50, 50], 0.5)])


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_and_library_agree_on_the_coco_symbols():
    from sylph_amd import _lib
    text = open(os.path.join(ROOT, "include", "sylph_hip.h")).read()
    for name, nargs in (("sylph_coco_match", 20), ("sylph_coco_accumulate", 18)):
        m = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"include/sylph_hip.h does not declare {name}"
        assert len(m.group(1).split(",")) == nargs
        assert len(_lib.PROTOTYPES[name][1]) == nargs
        assert hasattr(_lib.lib(), name)
    kernels = open(os.path.join(ROOT, "sylph-few-shot-detection_amd", "csrc", "kernels.h")).read()
    for const, value in (("COCO_MATCH_TILE_GT", _lib.COCO_MATCH_TILE_GT), ("COCO_ACC_CHUNK", _lib.COCO_ACC_CHUNK)):
        assert re.search(rf"^#define SYLPH_{const} {value}\b", text, re.M), f"include/sylph_hip.h does not define SYLPH_{const} as {value}"
        assert f"constexpr int {const} = {value};" in kernels
    assert re.search(r"int\s+sylph_coco_match_tile_gt\s*\(\s*int max_det\s*\)\s*;", text) and len(_lib.PROTOTYPES["sylph_coco_match_tile_gt"][1]) == 1


def test_tile_bound_shrinks_with_max_det():
    """the IoU tile is max_det x boxes float64 + 64 state bytes per box, next to 32 bytes per detection slot, in 144 KiB of LDS: the named
    bound holds up to max_det 131; the header's examples are what the library answers (a host function: no device)"""
    from sylph_amd import _lib
    tile = _lib.lib().sylph_coco_match_tile_gt
    fit = lambda md: min(_lib.COCO_MATCH_TILE_GT, (144 * 1024 - 32 * md) // (8 * md + 64))
    for md in (1, 100, 131, 132, 300, 1024):
        assert tile(md) == fit(md), md
    assert (tile(100), tile(131), tile(132), tile(300), tile(1024)) == (128, 128, 127, 55, 13)
    assert tile(0) == -1 and tile(1025) == -1
    text = open(os.path.join(ROOT, "include", "sylph_hip.h")).read()
    assert "55\n * boxes at max_det 300, 13 at 1024" in text or "55 boxes at max_det 300, 13 at 1024" in text


def test_header_cites_what_the_entries_replace():
    text = open(os.path.join(ROOT, "include", "sylph_hip.h")).read()
    assert "evaluateImg" in text and "meta_learn_evaluation.py:465" in text


# ---- DeviceCOCOEvaluator on the host ---------------------------------------------------------------------------------------------------
class _NoCpu(torch.Tensor):
    """a tensor that refuses the device -> host copy"""
    @staticmethod
    def __new__(cls, x):
        return torch.Tensor._make_subclass(cls, x)

    def cpu(self, *a, **k):
        raise AssertionError("process() copied detections to the host")

    def tolist(self):
        raise AssertionError("process() read detections on the host")


class _StubEngine:
    """stands where the Engine stands; every cell reports "no ground truth" """
    device = torch.device("cpu")

    def coco_match(self, rows, det_off, gt, n_cat, iou_thr, area_rng, max_det):
        z = torch.zeros(rows.shape[0], dtype=torch.int64)
        return z, z.clone(), torch.zeros(n_cat, area_rng.shape[0], dtype=torch.int32)

    def coco_accumulate(self, score, rank, matched, ignored, cat_off, npig, n_thr, rec_thr, max_dets):
        K, A, M, R = cat_off.numel() - 1, npig.shape[1], max_dets.numel(), rec_thr.numel()
        return -torch.ones(n_thr, R, K, A, M, dtype=torch.float64), -torch.ones(n_thr, K, A, M, dtype=torch.float64), \
            -torch.ones(n_thr, R, K, A, M, dtype=torch.float64)


def _outputs(n, seed, wrap=_NoCpu):
    from sylph_amd.structures import Boxes, Instances
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(n, 2, generator=g) * 50
    inst = Instances((100, 100), pred_boxes=Boxes(wrap(torch.cat([xy, xy + 10], dim=1))), scores=wrap(torch.rand(n, generator=g)),
                     pred_classes=wrap(torch.randint(1, 3, (n,), generator=g)))
    return {"instances": inst}


def test_process_appends_device_rows_without_a_host_copy():
    from sylph_amd.coco_eval import DeviceCOCOEvaluator
    gt = gt_of([(1, 1, [0, 0, 50, 50], None, 0), (2, 2, [0, 0, 50, 50], None, 0)], n_images=3, cats=(1, 2))
    ev = DeviceCOCOEvaluator(gt, engine=_StubEngine())
    ev.reset()
    ev.process([{"image_id": 2}, {"image_id": 1}], [_outputs(3, 0), _outputs(2, 1)])
    ev.process([{"image_id": 3}], [_outputs(0, 2)])
    assert [tuple(r.shape) for r in ev._rows] == [(5, 8), (0, 8)]
    assert isinstance(ev._rows[0], _NoCpu), "the rows are derived from the outputs' tensors"
    ev._rows = [r.as_subclass(torch.Tensor) for r in ev._rows]  # evaluate() may copy; process() has not
    assert ev._rows[0][:, 0].tolist() == [2, 2, 2, 1, 1] and bool((ev._rows[0][:, 7] == 1).all())
    res = ev.evaluate()["bbox"]
    assert list(res)[:12] == ["AP", "AP50", "AP75", "APs", "APm", "APl", "AR@1", "AR@10", "AR@100", "ARs", "ARm", "ARl"]
    assert list(res)[12:] == ["AP-c1", "AP-c2"] and all(math.isnan(v) for v in res.values())
    assert ev.precision.shape == (10, 101, 2, 4, 3) and ev.recall.shape == (10, 2, 4, 3) and ev.scores.shape == ev.precision.shape
    ev.reset()
    assert ev._rows == [] and ev.precision is None


def test_order_puts_pairs_then_scores_then_arrival():
    from sylph_amd.coco_eval import DeviceCOCOEvaluator
    gt = gt_of([(1, 1, [0, 0, 50, 50], None, 0)], n_images=2, cats=(1, 2))
    ev = DeviceCOCOEvaluator(gt, engine=_StubEngine())
    #                 image x0 y0 x1 y1 score class valid
    rows = torch.tensor([[2, 0, 0, 1, 1, 0.5, 1, 1], [1, 0, 0, 2, 2, 0.5, 2, 1], [2, 0, 0, 3, 3, 0.7, 1, 1], [0, 0, 0, 0, 0, 0, 0, 0],
                         [2, 0, 0, 4, 4, 0.5, 1, 1], [1, 0, 0, 5, 5, 0.9, 1, 1], [1, 0, 0, 6, 6, 0.2, 7, 1]], dtype=torch.float32)
    p = ev._order(rows)
    assert p["rows"][:, 3].tolist() == [5, 2, 3, 1, 4, 6, 0]  # (1, c1) | (1, c2) | (2, c1): 0.7, then the two 0.5 as they came | unknown class, padding
    assert p["det_off"].tolist() == [0, 1, 2, 5, 5] and p["rank"][:5].tolist() == [0, 0, 0, 1, 2]
    assert p["rows"][p["perm2"]][:, 3].tolist()[:5] == [5, 3, 1, 4, 2] and p["cat_off"].tolist() == [0, 4, 5]
    assert float(p["bad_id"]) == -1


def test_evaluator_refuses_an_unknown_image_id():
    from sylph_amd.coco_eval import DeviceCOCOEvaluator
    gt = gt_of([(1, 1, [0, 0, 50, 50], None, 0)])
    ev = DeviceCOCOEvaluator(gt, engine=_StubEngine())
    ev.reset()
    ev.process([{"image_id": 77}], [_outputs(2, 0, wrap=lambda x: x)])
    with pytest.raises(ValueError, match="77"):
        ev.evaluate()
    with pytest.raises(ValueError, match="not in the ground truth"):
        DeviceCOCOEvaluator(gt, category_subsets={"novel": [5]})
