"""LVIS bbox evaluation, host side (no GPU): hand-derivable known answers that pin the numpy restatement tests/lviseval_ref.py (the yardstick
of the GPU file; a restatement of lvis-api's protocol, not lvis-api), a cross-check of the two restatements where the two protocols
coincide, the C ABI's declarations and DeviceLVISEvaluator's host behaviour.  Every hit here is at IoU 1, every miss at IoU 0."""
import math
import os
import re

import numpy as np
import pytest
import torch

import cocoeval_ref as CR
import lviseval_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# "precision 1" of the protocol is tp / (tp + np.spacing(1)): one step below 1 where tp = 1, exactly 1 from tp = 2 on
ONE = pytest.approx(100.0, rel=1e-15)
A, B, FAR = [0, 0, 50, 50], [100, 100, 40, 40], [300, 300, 50, 50]


def gt_of(anns, n_images=1, cats=(1,), neg=None, nel=None, freq=None, names=None):
    """anns: (image id, category id, [x, y, w, h], ignore); neg / nel: {image id: [category ids]}; freq / names: {category id: ...}"""
    images = [{"id": i + 1, "neg_category_ids": list((neg or {}).get(i + 1, [])), "not_exhaustive_category_ids": list((nel or {}).get(i + 1, []))}
              for i in range(n_images)]
    categories = [{"id": c, "name": (names or {}).get(c, f"c{c}")} for c in cats]
    for c in categories:
        if freq and c["id"] in freq:
            c["frequency"] = freq[c["id"]]
    return {"images": images, "categories": categories,
            "annotations": [{"id": j + 1, "image_id": im, "category_id": c, "bbox": [float(v) for v in b], "area": float(b[2] * b[3]), "ignore": ig}
                            for j, (im, c, b, ig) in enumerate(anns)]}


def det(im, c, box, score):
    return {"image_id": im, "category_id": c, "bbox": [float(v) for v in box], "score": score}


# ---- known answers -------------------------------------------------------------------------------------------------------------------
def test_perfect_detections_give_one_everywhere():
    boxes = [[5, 5, 20, 20], [5, 5, 60, 60], [5, 5, 150, 150]]  # small, medium, large
    gt = gt_of([(i + 1, 1, b, 0) for i, b in enumerate(boxes)], n_images=3, freq={1: "f"})
    ev, res = LR.results(gt, [det(i + 1, 1, b, 0.9) for i, b in enumerate(boxes)])
    for k in ("AP", "AP50", "AP75", "APs", "APm", "APl", "APf", "AP-c1"):
        assert res[k] == ONE, k
    assert np.all(ev["recall"] == 1.0) and ev["precision"].shape == (10, 101, 1, 4) and ev["recall"].shape == (10, 1, 4)
    assert list(res) == list(LR.METRICS) + ["AP-c1"]


def _two_images(neg=None, nel=None):
    # category 2: a box with a perfect hit on image 2 (score 0.5) and a higher-scored detection far from everything on image 1
    gt = gt_of([(1, 1, A, 0), (2, 2, A, 0)], n_images=2, cats=(1, 2), neg=neg, nel=nel)
    return gt, [det(1, 2, FAR, 0.9), det(2, 2, A, 0.5), det(1, 1, A, 0.9)]


def test_miss_in_a_negative_category_halves_the_precision():
    _, res = LR.results(*_two_images(neg={1: [2]}))
    assert res["AP-c2"] == 50.0 and res["AP-c1"] == ONE  # fp, tp: precision 0, 1/2 -> 1/2 from the right at every recall threshold
    assert res["AP"] == pytest.approx(75.0, rel=1e-15)


def test_miss_in_a_category_neither_positive_nor_negative_changes_nothing():
    _, res = LR.results(*_two_images())
    assert res["AP-c2"] == ONE and res["AP"] == ONE
    gt, dets = _two_images()
    assert LR.results(gt, dets[1:])[1] == res  # the same numbers without the detection


def test_not_exhaustive_category_ignores_the_miss_and_counts_the_hit():
    anns = [(1, 1, A, 0)]
    dets = [det(1, 1, FAR, 0.9), det(1, 1, A, 0.8)]
    ev, res = LR.results(gt_of(anns, nel={1: [1]}), dets)
    assert res["AP"] == ONE and np.all(ev["recall"][:, 0, 0] == 1.0)  # the hit is a true positive, the miss neither
    m, ig, _, num_gt = LR.evaluate_img(gt_of(anns)["annotations"], [dict(d) for d in dets], CR.AREA_RNGS[0], True)
    assert not m[:, 0].any() and ig[:, 0].all() and m[:, 1].all() and not ig[:, 1].any() and num_gt == 1
    assert LR.results(gt_of(anns), dets)[1]["AP"] == 50.0  # exhaustively annotated: the miss is a false positive


def test_ignored_box_absorbs_a_detection():
    gt = gt_of([(1, 1, A, 0), (1, 1, B, 1)])
    dets = [det(1, 1, B, 0.9), det(1, 1, A, 0.5)]
    m, ig, _, num_gt = LR.evaluate_img(gt["annotations"], dets, CR.AREA_RNGS[0], False)
    assert m.all() and ig[:, 0].all() and not ig[:, 1].any() and num_gt == 1
    assert LR.results(gt, dets)[1]["AP"] == ONE  # as a false positive it would halve the precision
    gt["annotations"][1]["ignore"] = 0
    gt["annotations"][1]["bbox"] = [float(v) for v in FAR]  # now a second, unfound box and a plain false positive
    assert LR.results(gt, dets)[1]["AP50"] < 50.0


def test_the_301st_detection_of_an_image_is_cut_last_to_arrive_among_equal_scores():
    gt = gt_of([(1, 1, A, 0)])
    misses = [det(1, 1, FAR, 0.5) for _ in range(300)]
    _, res = LR.results(gt, misses + [det(1, 1, A, 0.5)])  # the hit arrives last: it is the one cut
    assert res["AP"] == 0.0
    ev, res = LR.results(gt, misses[:299] + [det(1, 1, A, 0.5), det(1, 1, FAR, 0.5)])  # the hit is the 300th
    assert res["AP"] == pytest.approx(100.0 / 300, rel=1e-12) and np.all(ev["recall"][:, 0, 0] == 1.0)
    assert LR.results(gt, misses + [det(1, 1, A, 0.5)], max_dets_per_image=301)[1]["AP"] == pytest.approx(100.0 / 301, rel=1e-12)


@pytest.mark.parametrize("other", [3, None])
def test_a_detection_that_is_filtered_out_later_still_uses_budget(other):
    """300 higher-scored detections of a category the image neither contains nor lists as negative (or of no category at all) push the
    only hit out of the budget; with 299 of them it stays"""
    gt = gt_of([(1, 1, A, 0)], cats=(1, 3))
    crowd = [det(1, other, FAR, 0.9) for _ in range(300)]
    assert LR.results(gt, crowd + [det(1, 1, A, 0.5)])[1]["AP-c1"] == 0.0
    assert LR.results(gt, crowd[1:] + [det(1, 1, A, 0.5)])[1]["AP-c1"] == ONE


def test_frequency_groups_select_their_categories():
    # rare: perfect; common: a negative-category miss before the hit; frequent: no detection at all; category 4 has no frequency
    gt = gt_of([(1, 1, A, 0), (1, 2, A, 0), (1, 3, A, 0), (1, 4, A, 0)], n_images=2, cats=(1, 2, 3, 4), neg={2: [2]}, freq={1: "r", 2: "c", 3: "f"})
    dets = [det(1, 1, A, 0.9), det(2, 2, FAR, 0.9), det(1, 2, A, 0.5), det(1, 4, A, 0.5)]
    _, res = LR.results(gt, dets)
    assert res["APr"] == ONE and res["APc"] == 50.0 and res["APf"] == 0.0
    assert res["AP"] == pytest.approx(62.5, rel=1e-15)  # all four categories


def test_empty_frequency_group_reads_minus_100():
    gt = gt_of([(1, 1, A, 0)], freq={1: "c"})
    _, res = LR.results(gt, [det(1, 1, A, 0.9)])
    assert res["APr"] == -100.0 and res["APf"] == -100.0 and res["APc"] == ONE
    assert res["APs"] == -100.0 and res["APl"] == -100.0 and res["APm"] == ONE  # 50 x 50 = 2500 lies in [32^2, 96^2] alone


def test_short_name_and_its_overwrite():
    assert LR.short_name("abcdefghijklm") == "abcdefghijklm" and LR.short_name("abcdefghijklmn") == "abcdefghijk.."
    names = {1: "abcdefghijkXYZ", 2: "thirteen_char", 3: "abcdefghijklmnop"}
    gt = gt_of([(1, 1, A, 0), (1, 2, A, 0), (1, 3, A, 0)], cats=(1, 2, 3), names=names)
    _, res = LR.results(gt, [det(1, 1, A, 0.9), det(1, 2, A, 0.9)])  # category 3, undetected, shares category 1's short name
    assert list(res)[9:] == ["AP-abcdefghijk..", "AP-thirteen_char"]
    assert res["AP-abcdefghijk.."] == 0.0 and res["AP-thirteen_char"] == ONE  # the later category overwrote 100


def test_category_without_non_ignored_ground_truth_reports_nan():
    gt = gt_of([(1, 1, A, 0), (1, 2, A, 1)], cats=(1, 2))
    ev, res = LR.results(gt, [det(1, 1, A, 0.9), det(1, 2, A, 0.9)])
    assert np.all(ev["precision"][:, :, 1] == -1) and np.all(ev["recall"][:, 1] == -1)
    assert math.isnan(res["AP-c2"]) and res["AP-c1"] == ONE and res["AP"] == ONE


# ---- the two restatements where the protocols coincide -----------------------------------------------------------------------------------
def lvis_dets(dets, cats):
    """{image id: (n, 6) fp32 rows x0 y0 x1 y1 score class} -> result dicts, widened as detection_rows_to_coco widens device rows"""
    out = []
    for im in dets:
        for x0, y0, x1, y1, s, c in dets[im].astype(np.float64).tolist():
            out.append({"image_id": im, "category_id": cats[int(c)], "bbox": [x0, y0, x1 - x0, y1 - y0], "score": s})
    return out


def test_lvis_and_coco_restatements_agree_without_federation():
    """no ignore, no crowd, every category negative wherever it is not positive, nothing not-exhaustive, at most 300 detections per image:
    the LVIS protocol is the COCO one with a single maxDet of 300"""
    from test_coco_eval_gpu import make_case
    ims, cats = [10 + 3 * i for i in range(12)], [1, 3, 4, 7, 20, 90]
    gt, dets = make_case(7, ims, cats, gt_per_pair=lambda r, im, c: 0 if c == 90 or r.random() < 0.25 else r.integers(1, 6),
                         det_per_pair=lambda r, im, c: 0 if r.random() < 0.2 else r.integers(1, 14), crowd=0.0)
    for im in gt["images"]:
        im["neg_category_ids"] = list(cats)
    rows = lvis_dets(dets, cats)
    assert max(len(d) for d in dets.values()) <= 300 and not any(a["iscrowd"] for a in gt["annotations"])
    lv, co = LR.evaluate(gt, rows), CR.evaluate(gt, rows, max_dets=(300,))
    assert np.array_equal(lv["precision"].view(np.int64), np.ascontiguousarray(co["precision"][..., 0]).view(np.int64))
    assert np.array_equal(lv["recall"].view(np.int64), np.ascontiguousarray(co["recall"][..., 0]).view(np.int64))
    assert (lv["precision"] > 0).any() and np.all(lv["precision"][:, :, 5] == -1)
    for im in gt["images"]:  # and federation matters: without the lists, detections of a category the image does not hold are dropped
        im["neg_category_ids"] = []
    assert not np.array_equal(LR.evaluate(gt, rows)["precision"], lv["precision"])


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_and_library_agree_on_the_lvis_symbols():
    from sylph_amd import _lib
    text = open(os.path.join(ROOT, "include", "sylph_hip.h")).read()
    m = re.search(r"int\s+sylph_lvis_match\s*\(([^;]*)\)\s*;", text)
    assert m and len(m.group(1).split(",")) == 23 and len(_lib.PROTOTYPES["sylph_lvis_match"][1]) == 23 and hasattr(_lib.lib(), "sylph_lvis_match")
    assert re.search(r"int\s+sylph_lvis_match_fits\s*\(\s*int n_det\s*,\s*int n_gt\s*\)\s*;", text) and len(_lib.PROTOTYPES["sylph_lvis_match_fits"][1]) == 2
    kernels = open(os.path.join(ROOT, "sylph-few-shot-detection_amd", "csrc", "kernels.h")).read()
    assert re.search(rf"^#define SYLPH_LVIS_MATCH_SLICE_BYTES {_lib.LVIS_MATCH_SLICE_BYTES}\b", text, re.M)
    assert re.search(rf"^#define SYLPH_LVIS_MATCH_MAX_DETS {_lib.LVIS_MATCH_MAX_DETS}\b", text, re.M)
    assert "constexpr int LVIS_MATCH_SLICE_BYTES = 36 * 1024;" in kernels and _lib.LVIS_MATCH_SLICE_BYTES == 36 * 1024
    assert f"constexpr int LVIS_MATCH_MAX_DETS = {_lib.LVIS_MATCH_MAX_DETS};" in kernels


def test_fits_follows_the_slice_formula_and_is_monotone():
    """a pair's 32-byte detection boxes, its D x G float64 tile and its 64-byte state rows in one wave's 36 KiB: a host function, no device"""
    from sylph_amd import _lib
    fits = _lib.lib().sylph_lvis_match_fits
    formula = lambda d, g: int(32 * d + g * (8 * d + 64) <= _lib.LVIS_MATCH_SLICE_BYTES)
    ds, gs = [0, 1, 2, 63, 64, 65, 299, 300, 301, 1000, 1024], [0, 1, 3, 4, 10, 11, 12, 59, 60, 61, 510, 511, 512, 576, 577, 5000]
    for d in ds:
        for g in gs:
            assert fits(d, g) == formula(d, g), (d, g)
    for d in ds:
        assert [fits(d, g) for g in gs] == sorted([fits(d, g) for g in gs], reverse=True)  # once a count does not fit, no larger one does
    for g in gs:
        assert [fits(d, g) for d in ds] == sorted([fits(d, g) for d in ds], reverse=True)
    assert (fits(300, 11), fits(300, 12), fits(64, 60), fits(64, 61), fits(1, 511), fits(1, 512)) == (1, 0, 1, 0, 1, 0)  # the header's examples
    assert fits(-1, 0) == -1 and fits(0, -1) == -1 and fits(1025, 0) == -1


def test_header_cites_what_the_entry_replaces():
    text = open(os.path.join(ROOT, "include", "sylph_hip.h")).read()
    assert "sylph/evaluation/lvis_evaluation.py:246-250" in text and "evaluate_img" in text and "limit_dets_per_image" in text
    assert "D = 300 fits 11 boxes, D = 64 fits 60, D = 1 fits 511" in text


# ---- DeviceLVISEvaluator on the host ---------------------------------------------------------------------------------------------------
def test_category_restriction_drops_images_without_kept_annotations():
    from sylph_amd.lvis_eval import DeviceLVISEvaluator
    gt = gt_of([(1, 1, A, 0), (2, 2, A, 0), (3, 1, B, 0), (3, 2, A, 0)], n_images=4, cats=(1, 2, 5), neg={2: [1]})
    ev = DeviceLVISEvaluator(gt, category_ids=[1, 5])
    assert ev.image_ids == [1, 3] and ev.cat_ids == [1, 5] and ev._gt_host["box"].shape == (2, 4)
    assert DeviceLVISEvaluator(gt).image_ids == [1, 2, 3, 4]
    images, anns, cats = LR.index(gt, [1, 5])
    assert [im["id"] for im in images] == [1, 3] and len(anns) == 2 and [c["id"] for c in cats] == [1, 5]
    with pytest.raises(ValueError, match="image id 2"):
        LR.evaluate(gt, [det(2, 1, A, 0.5)], category_ids=[1, 5])  # image 2 lists category 1 as negative, but holds no kept annotation
    rows = torch.tensor([[2, 0, 0, 50, 50, 0.5, 1, 1]], dtype=torch.float32)
    assert float(ev._order(rows)["bad_id"]) == 2 and float(DeviceLVISEvaluator(gt)._order(rows)["bad_id"]) == -1
    with pytest.raises(ValueError, match="not in the ground truth"):
        DeviceLVISEvaluator(gt, category_ids=[1, 5], category_subsets={"novel": [2]})
    with pytest.raises(ValueError, match="LVIS_MATCH_MAX_DETS"):
        DeviceLVISEvaluator(gt, max_dets_per_image=1025)


def test_order_applies_budget_and_federation_and_lists_only_live_pairs():
    from sylph_amd.lvis_eval import DeviceLVISEvaluator
    gt = gt_of([(1, 1, A, 0), (2, 2, A, 0)], n_images=2, cats=(1, 2, 3), neg={1: [2]}, nel={2: [2]})
    ev = DeviceLVISEvaluator(gt, max_dets_per_image=3)
    #                 image x0 y0 x1 y1 score class valid
    rows = torch.tensor([[2, 0, 0, 1, 1, 0.5, 2, 1], [1, 0, 0, 2, 2, 0.5, 2, 1], [1, 0, 0, 3, 3, 0.7, 3, 1], [0, 0, 0, 0, 0, 0, 0, 0],
                         [1, 0, 0, 4, 4, 0.9, 1, 1], [1, 0, 0, 5, 5, 0.5, 2, 1], [2, 0, 0, 6, 6, 0.2, 7, 1], [2, 0, 0, 7, 7, 0.9, 2, 1]],
                        dtype=torch.float32)
    p = ev._order(rows)
    # (1, c1) | (1, c2) | (2, c2): 0.9 then 0.5 | dropped, image by image: category 3 is neither positive nor negative on image 1 (but took
    # budget, so the second 0.5 of (1, c2) is the image's fourth row and cut), class 7 has no category; then the padding row
    assert p["rows"][:, 3].tolist() == [4, 2, 7, 1, 3, 5, 6, 0]
    q = p["pairs"]
    assert q["n"].tolist() == [3] and q["cat"].numel() == 8 + 2, "sized by rows + ground-truth pairs, the live count apart"
    assert p["pair_key"][:3].tolist() == [0, 1, 4] and q["cat"][:3].tolist() == [0, 1, 1] and q["flags"][:3].tolist() == [0, 0, 1]
    assert q["det_off"][:4].tolist() == [0, 1, 2, 4] and q["gt_off"][:4].tolist() == [0, 1, 1, 2] and p["rank"][:4].tolist() == [0, 0, 0, 1]
    assert p["rows"][p["perm2"]][:, 3].tolist()[:4] == [4, 7, 2, 1] and p["cat_off"].tolist() == [0, 1, 4, 4]
    assert float(p["bad_id"]) == -1
    empty = ev._order(torch.zeros(0, 8))
    assert empty["pairs"]["n"].tolist() == [2] and empty["pairs"]["gt_off"][:3].tolist() == [0, 1, 2] and empty["pairs"]["det_off"][:3].tolist() == [0, 0, 0]


def test_pair_keys_past_2_to_31_are_not_refused():
    from sylph_amd.lvis_eval import DeviceLVISEvaluator
    """50 000 images x 50 000 categories: 2.5e9 pairs, of which two exist; the keys are int64 and no table has an entry per pair"""
    n = 50000
    gt = {"images": [{"id": i} for i in range(n)], "categories": [{"id": c, "name": str(c)} for c in range(n)],
          "annotations": [{"id": 1, "image_id": n - 1, "category_id": n - 1, "bbox": [0.0, 0.0, 5.0, 5.0], "area": 25.0}]}
    gt["images"][n - 2]["neg_category_ids"] = [n - 3]
    ev = DeviceLVISEvaluator(gt)
    rows = torch.tensor([[n - 1, 0, 0, 5, 5, 0.5, n - 1, 1], [n - 2, 0, 0, 5, 5, 0.5, n - 3, 1], [n - 2, 0, 0, 5, 5, 0.9, n - 4, 1]], dtype=torch.float32)
    p = ev._order(rows)
    assert p["pairs"]["n"].tolist() == [2] and p["pair_key"][:2].tolist() == [(n - 2) * n + n - 3, (n - 1) * n + n - 1]
    assert p["pair_key"][1] > (1 << 31) and p["pairs"]["cat"][:2].tolist() == [n - 3, n - 1] and p["pairs"]["cat"].numel() == 3 + 1
    assert p["pairs"]["det_off"][:3].tolist() == [0, 1, 2] and p["pairs"]["gt_off"][:3].tolist() == [0, 0, 1]
