"""LVIS bbox evaluation on the GPU: DeviceLVISEvaluator (torch plumbing over int64 pair keys, lvis_match_kernel over the compacted pair list,
coco_accumulate_kernel with one unbounded maxDet) against the float64 numpy restatement tests/lviseval_ref.py -- a restatement of lvis-api's
protocol, not lvis-api.

The criterion is BIT equality of precision [T, R, K, A] and recall [T, K, A] and equal result dicts with NaN at the same keys: every
operation on the way is one IEEE float64 add, multiply, divide or compare in a fixed order, so there is no tolerance.  The restatement
sees detection_rows_to_coco of the very rows the evaluator holds.

The cases come from test_coco_eval_gpu.make_case: a half-pixel grid, widths that are multiples of 3 or 7, detections shifted by a third or
a seventh of a width, eight fp32 score values -- IoUs of exactly 0.5 and 0.75, IoU ties and score ties occur (asserted below)."""
import math

import numpy as np
import pytest
import torch

import cocoeval_ref as CR
import lviseval_ref as LR
from sylph_amd import _lib
from sylph_amd.evaluation import detection_rows_to_coco
from test_coco_eval_gpu import _bits, _feed, make_case

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def engine():
    from sylph_amd.engine import Engine
    eng = Engine(None, dtype="f32")
    yield eng
    eng.close()


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
def lvis_case(seed, ims, cats, gt_per_pair, det_per_pair, ignore=0.15, federate=True, pair_fill=0.7):
    """make_case without crowd boxes, turned into an LVIS set: ignore flags on some annotations (the key is absent on others), per image a
    random part of the categories it does not hold as negatives (the rest: neither), a random part of all as not exhaustively annotated, and
    frequencies r / c / f in turn with every fourth category left without one.  federate=False: every category negative everywhere."""
    gt, dets = make_case(seed, ims, cats, gt_per_pair, det_per_pair, crowd=0.0, pair_fill=pair_fill)
    rng = np.random.default_rng(seed + 1000)
    for a in gt["annotations"]:
        del a["iscrowd"]
        if rng.random() < ignore:
            a["ignore"] = 1
        elif rng.random() < 0.5:
            a["ignore"] = 0
    for im in gt["images"]:
        pos = {a["category_id"] for a in gt["annotations"] if a["image_id"] == im["id"]}
        im["neg_category_ids"] = [c for c in cats if c not in pos and (not federate or rng.random() < 0.6)]
        if federate:
            im["not_exhaustive_category_ids"] = [c for c in cats if rng.random() < 0.25]
    for k, c in enumerate(gt["categories"]):
        if k % 4 < 3:
            c["frequency"] = "rcf"[k % 4]
    return gt, dets


def _assert_equal(ev, res, gt, c2d, what, rows=None, pairs=None, **kw):
    rows = torch.cat(ev._rows) if rows is None else rows
    want_ev, want = LR.results(gt, detection_rows_to_coco(rows, c2d), kw.get("category_ids"), kw.get("max_dets_per_image", 300),
                               kw.get("category_subsets"), pairs)
    for name in ("precision", "recall"):
        got = getattr(ev, name)
        assert got.shape == want_ev[name].shape and got.dtype == np.float64, f"{what}: {name} shape / dtype"
        diff = np.argwhere(_bits(got) != _bits(want_ev[name]))
        assert diff.size == 0, (f"{what}: {name} differs at {len(diff)} of {got.size} entries, first {tuple(diff[0])}: "
                                f"{got[tuple(diff[0])]!r} for {want_ev[name][tuple(diff[0])]!r}")
    got = res["bbox"]
    assert list(got) == list(want), f"{what}: keys"
    for k in want:
        assert (math.isnan(got[k]) and math.isnan(want[k])) or got[k] == want[k], f"{what}: {k}: {got[k]!r} for {want[k]!r}"
    return want_ev, want


def _run(engine, gt, dets, cats, what, batch=7, seed=0, c2d=None, pairs=None, **kw):
    from sylph_amd.lvis_eval import DeviceLVISEvaluator
    c2d = {k: c for k, c in enumerate(cats)} if c2d is None else c2d
    ev = DeviceLVISEvaluator(gt, contiguous_to_dataset_id=c2d, engine=engine, **kw)
    order = [int(i) for i in np.random.default_rng(seed).permutation(sorted(dets))]
    _feed(ev, dets, order, batch)
    res = ev.evaluate()
    return ev, res, _assert_equal(ev, res, gt, c2d, what, pairs=pairs, **kw)


def _xywh(r):
    return [float(r[0]), float(r[1]), float(r[2]) - float(r[0]), float(r[3]) - float(r[1])]


# ---- the federated rules ----------------------------------------------------------------------------------------------------------------------
def test_federated_rules_in_one_launch(engine):
    """6 images x 4 categories: a detection dropped because its category is neither positive nor negative, a false positive in a negative
    category, unmatched and matched detections in a not exhaustively annotated category, pairs with one side empty, an image with nothing"""
    from sylph_amd.coco_eval import DeviceCOCOEvaluator
    ims, cats = [1, 2, 3, 4, 5, 6], [2, 4, 6, 8]
    G = {(1, 2), (2, 4), (3, 6), (6, 2), (6, 8)}
    D = {(1, 2), (1, 4), (1, 6), (2, 4), (4, 8), (6, 2), (6, 8)}
    gt, dets = make_case(3, ims, cats, gt_per_pair=lambda r, im, c: 2 if (im, c) in G else 0, det_per_pair=lambda r, im, c: 5 if (im, c) in D else 0,
                         crowd=0.0)
    for a in gt["annotations"]:
        del a["iscrowd"]
    neg, nel = {1: [4], 4: [8]}, {2: [4], 6: [8]}
    for im in gt["images"]:
        im["neg_category_ids"], im["not_exhaustive_category_ids"] = neg.get(im["id"], []), nel.get(im["id"], [])
    ev, res, (want_ev, want) = _run(engine, gt, dets, cats, "federated rules", batch=2)
    assert dets[5].shape[0] == 0 and dets[3].shape[0] == 0 and dets[1].shape[0] == 15
    # every rule fires: (2, 4) holds matched and unmatched detections under the not-exhaustive flag ...
    rows24 = sorted((r for r in dets[2].tolist()), key=lambda r: -r[4])
    m, ig, _, _ = LR.evaluate_img([a for a in gt["annotations"] if a["image_id"] == 2], [{"bbox": _xywh(r), "score": r[4]} for r in rows24],
                                  CR.AREA_RNGS[0], True)
    assert m[0].any() and (~m[0]).any() and ig[0][~m[0]].all() and not ig[0][m[0]].any()
    # ... category 4 has exactly (1, 4)'s five false positives next to (2, 4), and (1, 6) is dropped: category 6 reads recall 0, precision 0
    k4, k6 = cats.index(4), cats.index(6)
    assert want_ev["recall"][0, k4, 0] > 0 and want["AP-cat4"] < 100 and np.all(want_ev["precision"][:, :, k6, 0] == 0)
    without = dict(dets)
    without[1] = dets[1][dets[1][:, 5] != float(k6)]
    assert _run(engine, gt, without, cats, "without the dropped rows", batch=2)[1] == res
    # the rules are not vacuous: the COCO protocol on the same data gives other numbers
    coco = DeviceCOCOEvaluator(gt, contiguous_to_dataset_id={k: c for k, c in enumerate(cats)}, max_dets=(300,), engine=engine)
    _feed(coco, dets, ims, 2)
    coco.evaluate()
    assert coco.precision[..., 0].shape == ev.precision.shape and not np.array_equal(coco.precision[..., 0], ev.precision)


# ---- the per-image budget --------------------------------------------------------------------------------------------------------------------
def test_301_detections_over_three_categories(engine):
    """the default budget of 300 cuts the image's lowest-scored row, the last to arrive among equal scores, whatever its category"""
    ims, cats = [4, 6], [7, 8, 9]
    per = {7: 100, 8: 100, 9: 101}
    gt, dets = lvis_case(5, ims, cats, gt_per_pair=lambda r, im, c: 4, det_per_pair=lambda r, im, c: per[c] if im == 4 else 6, federate=False)
    s = np.sort(dets[4][:, 4])[::-1]
    assert dets[4].shape[0] == 301 and s[299] == s[300], "a score tie across the boundary"
    ev, res, _ = _run(engine, gt, dets, cats, "301 detections", batch=1)
    mine = [d for d in detection_rows_to_coco(torch.cat(ev._rows), {k: c for k, c in enumerate(cats)}) if d["image_id"] == 4]
    kept = LR.limit_dets_per_image(mine, 300)
    last_lowest = [d for d in mine if d["score"] == float(s[300])][-1]
    assert len(kept) == 300 and not any(d is last_lowest for d in kept), "the restatement cuts the last arrival among the lowest scores"
    _run(engine, gt, dets, cats, "budget 301", batch=1, max_dets_per_image=301)


def test_class_without_category_takes_budget(engine):
    ims, cats = [4, 6, 9], [7, 8]
    gt, dets = lvis_case(6, ims, cats, gt_per_pair=3, det_per_pair=6, federate=False, pair_fill=1.0)
    c2d = {0: 7, 1: 8, 2: None}
    base = _run(engine, gt, dets, cats, "budget 8", c2d=c2d, max_dets_per_image=8)[0]
    more = {im: np.concatenate([np.array([[5, 5, 50, 50, 0.9375, 2]] * 4, dtype=np.float32), d]) for im, d in dets.items()}
    ev = _run(engine, gt, more, cats, "budget 8 with four rows of a class that has no category", c2d=c2d, max_dets_per_image=8)[0]
    assert not np.array_equal(ev.precision, base.precision), "they pushed four rows of every image out of its budget"
    same = _run(engine, gt, more, cats, "budget 300 with them", c2d=c2d)[0]
    assert np.array_equal(same.precision, _run(engine, gt, dets, cats, "budget 300", c2d=c2d)[0].precision), "and change nothing under a wide budget"


# ---- pair shapes: tile or recompute, decided per pair ------------------------------------------------------------------------------------------
def _largest_fitting(D):
    fits = _lib.lib().sylph_lvis_match_fits
    g = 1
    while fits(D, g + 1) == 1:
        g += 1
    return g


@pytest.mark.parametrize("D", [1, 64, 65, 300])
@pytest.mark.parametrize("which", ["one", "largest", "largest + 1"])
def test_pair_shapes(engine, D, which):
    """D detections against 1 box, the most boxes whose tile fits the wave's slice next to D detections, and one more (no tile: the IoU is
    recomputed and the state rows live in the scratch); D = 300 is a pair that holds its image's whole budget.  A second, small pair rides
    along so that both paths run in the launch past the bound"""
    gmax = _largest_fitting(D)
    assert gmax == {1: 511, 64: 60, 65: 59, 300: 11}[D] == (_lib.LVIS_MATCH_SLICE_BYTES - 32 * D) // (8 * D + 64)
    G = {"one": 1, "largest": gmax, "largest + 1": gmax + 1}[which]
    ims, cats = [1, 2], [1]
    gt, dets = lvis_case(100 * D + G, ims, cats, gt_per_pair=lambda r, im, c: G if im == 1 else 1,
                         det_per_pair=lambda r, im, c: D if im == 1 else 5, federate=False)
    ev, res, (want_ev, _) = _run(engine, gt, dets, cats, f"D = {D}, G = {G}", batch=1)
    assert ev._tables(DEV)["max_per_pair"] == G and dets[1].shape[0] == D
    assert _lib.lib().sylph_lvis_match_fits(D, G) == (0 if which == "largest + 1" else 1)
    assert D == 1 or want_ev["recall"][0, 0, 0] > 0, "something matches"


def test_match_without_scratch_is_refused_before_any_launch(engine):
    """the C entry with a NULL scratch and bounds under which a pair may not fit fails by name on the host: nothing is launched"""
    from ctypes import c_void_p
    from sylph_amd.engine import _ptr
    z = lambda *shape, dt=torch.float64: torch.zeros(*shape, dtype=dt, device=DEV)
    off, one, thr, rng = z(2, dt=torch.int32), z(1, dt=torch.int32), z(10), z(4, 2)
    box, area, ign, npig = z(100, 4), z(100), z(100, dt=torch.int32), z(1, 4, dt=torch.int32)
    call = lambda max_det, max_gt: engine.L.sylph_lvis_match(
        engine._ctx, 0, c_void_p(0), 1, _ptr(one), 1, _ptr(one), _ptr(one), _ptr(off), _ptr(box), _ptr(area), _ptr(ign), _ptr(off), max_gt, 10,
        _ptr(thr), 4, _ptr(rng), max_det, c_void_p(0), c_void_p(0), c_void_p(0), _ptr(npig))
    for max_det, max_gt in ((300, 12), (64, 61), (1, 512)):
        assert call(max_det, max_gt) != 0
        assert b"gt_scratch_dev" in engine.L.sylph_last_error() and b"sylph_lvis_match_fits" in engine.L.sylph_last_error()
    assert call(1025, 1) != 0 and b"LVIS_MATCH_MAX_DETS" in engine.L.sylph_last_error()
    assert call(300, 11) == 0, engine.L.sylph_last_error()  # at the bound no scratch is needed (live count 0: the one wave returns at once)
    torch.cuda.synchronize()


# ---- the seeded random set --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_set():
    ims, cats = [10 + 3 * i for i in range(40)], [1, 3, 4, 7, 20, 90, 91]
    rng = np.random.default_rng(99)
    empty = {int(i) for i in rng.choice(ims, 3, replace=False)}
    # category 90: no ground truth at all but detections; category 91 ("a_long_category_name"): ignored ground truth only
    gt, dets = lvis_case(7, ims, cats, gt_per_pair=lambda r, im, c: 0 if im in empty or c == 90 or r.random() < 0.25 else r.integers(1, 6),
                         det_per_pair=lambda r, im, c: 0 if im in empty or r.random() < 0.2 else r.integers(1, 14))
    for a in gt["annotations"]:
        if a["category_id"] == 91:
            a["ignore"] = 1
    gt["categories"][6]["name"] = "a_long_category_name"
    # an exact IoU tie: a detection halfway between two equal boxes of its pair (10 / 14 with each), away from everything else
    im0, n = next(im for im in ims if im not in empty), len(gt["annotations"])
    gt["annotations"] += [{"id": n + 1 + j, "image_id": im0, "category_id": 1, "bbox": [400.0 + 4 * j, 400.0, 12.0, 12.0], "area": 144.0} for j in range(2)]
    dets[im0] = np.concatenate([dets[im0], np.array([[402, 400, 414, 412, 0.9375, 0]], dtype=np.float32)])
    return ims, cats, gt, dets


@pytest.mark.parametrize("batch", [1, 7])
def test_random_set_shuffled(engine, random_set, batch):
    """ignore flags, areas that are not w * h on both sides of 32^2 and 96^2, ignored boxes ahead of non-ignored ones in file order, frequency
    groups, and every federated rule, in shuffled process() order"""
    ims, cats, gt, dets = random_set
    ev, res, (want_ev, want) = _run(engine, gt, dets, cats, f"random set, batches of {batch}", batch=batch, seed=batch)
    anns = gt["annotations"]
    assert any(a.get("ignore") for a in anns) and any("ignore" not in a for a in anns)
    areas = [a["area"] for a in anns if a["area"] != a["bbox"][2] * a["bbox"][3]]
    assert min(areas) < 32 ** 2 < max(areas) and any(32 ** 2 < x < 96 ** 2 for x in areas) and max(areas) > 96 ** 2
    assert any(a["area"] < 32 ** 2 <= a["bbox"][2] * a["bbox"][3] for a in anns) and any(a["area"] < 96 ** 2 <= a["bbox"][2] * a["bbox"][3] for a in anns)
    first = {}
    for a in anns:  # file order inside a pair
        first.setdefault((a["image_id"], a["category_id"]), []).append(bool(a.get("ignore")))
    assert any(f[0] and not all(f) for f in first.values()), "an ignored box comes before a non-ignored one of its pair"
    rows = torch.cat(ev._rows).cpu().numpy()
    assert len(np.unique(rows[:, 5])) == 8, "eight score values: ties everywhere"
    k90, k91 = cats.index(90), cats.index(91)
    assert np.all(want_ev["precision"][:, :, [k90, k91]] == -1) and math.isnan(want["AP-cat90"]) and math.isnan(want["AP-a_long_cate.."])
    assert 0 < want["AP"] < 100 and 0 < want["AP75"] < want["AP50"]
    assert all(want[k] >= 0 for k in ("APr", "APc", "APf")) and len({want["APr"], want["APc"], want["APf"]}) == 3
    ious = [CR.iou(_xywh(r), a["bbox"], False) for im in ims[:10] for r in dets[im].tolist() for a in anns if a["image_id"] == im]
    assert 0.5 in ious and 0.75 in ious, "IoUs exactly at a threshold occur"
    tied = [len(v) - len(set(v)) for im in ims for r in dets[im].tolist()
            for v in [[x for x in (CR.iou(_xywh(r), a["bbox"], False) for a in anns if a["image_id"] == im and a["category_id"] == cats[int(r[5])]) if x > 0]]]
    assert max(tied) > 0, "a detection overlaps two boxes of its pair equally"


def test_small_budget_on_the_random_set(engine, random_set):
    ims, cats, gt, dets = random_set
    ev, res, _ = _run(engine, gt, dets, cats, "budget 5", max_dets_per_image=5)
    assert max(d.shape[0] for d in dets.values()) > 5


def test_category_restriction_and_subsets(engine, random_set):
    ims, cats, gt, dets = random_set
    subsets = {"novel": [3, 20, 90], "base": [1, 4, 7]}
    ev, res, (_, want) = _run(engine, gt, dets, cats, "subsets", category_subsets=subsets)
    assert all(k in res["bbox"] for k in ("nAP", "nAP50", "nAPr", "nAPf", "bAP", "bAPl", "bAPc")) and res["bbox"]["nAP"] != res["bbox"]["bAP"]
    # categories 1, 4 and 7 are rare, frequent and without a frequency; 3, 20 and 90 common, rare and common
    assert res["bbox"]["bAPc"] == -100.0 and res["bbox"]["nAPf"] == -100.0 and res["bbox"]["bAPr"] >= 0 and res["bbox"]["nAPc"] >= 0
    keep = [1, 4, 20]
    held = {a["image_id"] for a in gt["annotations"] if a["category_id"] in keep}
    some = {im: d for im, d in dets.items() if im in held}
    assert len(some) < len(dets)
    ev, res, _ = _run(engine, gt, some, cats, "category_ids", category_ids=keep)
    assert ev.precision.shape[2] == 3 and ev.image_ids == sorted(held)


def test_padding_rows_in_the_middle(engine, random_set):
    """gather_detection_rows pads every rank's block with valid = 0 rows: two blocks, the first half full"""
    from sylph_amd.evaluation import gather_detection_rows
    from sylph_amd.lvis_eval import DeviceLVISEvaluator
    ims, cats, gt, dets = random_set
    c2d = {k: c for k, c in enumerate(cats)}
    ev = DeviceLVISEvaluator(gt, contiguous_to_dataset_id=c2d, engine=engine)
    _feed(ev, dets, ims[::-1], 7)
    rows = torch.cat(ev._rows)
    half = rows.shape[0] // 2
    blocks = [gather_detection_rows(rows[:half], half + 300), gather_detection_rows(rows[half:], half + 300)]
    assert float(blocks[0][half:, 7].sum()) == 0 and blocks[0].shape[0] == half + 300
    ev._rows = blocks
    _assert_equal(ev, ev.evaluate(), gt, c2d, "padding rows", rows=rows)


def test_distributed_flag_on_one_rank(engine, random_set):
    ims, cats, gt, dets = random_set
    _run(engine, gt, {im: dets[im] for im in ims[:8]}, cats, "distributed, one rank", batch=2, distributed=True)


def test_evaluator_with_its_own_engine_and_refusals(random_set):
    from sylph_amd.lvis_eval import DeviceLVISEvaluator
    ims, cats, gt, dets = random_set
    c2d = {k: c for k, c in enumerate(cats)}
    ev = DeviceLVISEvaluator(gt, contiguous_to_dataset_id=c2d)
    _feed(ev, dets, ims[:6], 2)
    _assert_equal(ev, ev.evaluate(), gt, c2d, "own engine")
    ev.reset()
    assert ev.evaluate()["bbox"]["AP"] == 0.0  # no detections at all: recall 0, precision 0 wherever there is ground truth
    bad = dict(dets)
    bad[5] = dets[ims[0]]
    _feed(ev, bad, [ims[1], 5], 2)
    with pytest.raises(ValueError, match="image id 5"):
        ev.evaluate()
    with pytest.raises(ValueError, match="LVIS_MATCH_MAX_DETS"):
        DeviceLVISEvaluator(gt, contiguous_to_dataset_id=c2d, max_dets_per_image=_lib.LVIS_MATCH_MAX_DETS + 1, engine=ev.engine)
    ev.engine.close()


# ---- the sparse pair table --------------------------------------------------------------------------------------------------------------------
def test_sparse_table_of_24_million_pairs(engine):
    """20 000 image ids x 1 203 categories, of which some dozens of pairs exist.  The peak device allocation during evaluate() stays under
    32 MiB: one dense int32 table of that many pairs alone is 96 MB, so the cap tells a compacted pair list from a dense one"""
    from sylph_amd.lvis_eval import DeviceLVISEvaluator
    n_img, cats = 20000, list(range(1, 1204))
    rng = np.random.default_rng(17)
    live_ims = sorted(int(i) for i in rng.choice(n_img, 24, replace=False)) + [n_img - 1]
    live_cats = sorted(int(c) for c in rng.choice(cats, 9, replace=False)) + [1203]
    small, dets = lvis_case(23, live_ims, live_cats, gt_per_pair=lambda r, im, c: r.integers(1, 3) if r.random() < 0.15 else 0,
                            det_per_pair=lambda r, im, c: r.integers(1, 8) if r.random() < 0.4 else 0)
    by_id = {im["id"]: im for im in small["images"]}
    gt = {"images": [by_id.get(i, {"id": i}) for i in range(n_img)], "annotations": small["annotations"],
          "categories": [{"id": c, "name": f"cat{c}", "frequency": "rcf"[c % 3]} for c in cats]}
    c2d = {k: c for k, c in enumerate(live_cats)}
    n_rows = sum(d.shape[0] for d in dets.values())
    assert 0 < n_rows < 1000 and 0 < len(gt["annotations"]) < 100 and n_img * len(cats) > 23.8e6
    ev = DeviceLVISEvaluator(gt, contiguous_to_dataset_id=c2d, engine=engine)
    _feed(ev, dets, live_ims, 7)
    ev._tables(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    res = ev.evaluate()
    peak = torch.cuda.max_memory_allocated() - before
    print(f"peak device allocation during evaluate(): {peak / 2 ** 20:.1f} MiB")
    assert peak < 32 * 2 ** 20
    pairs = [(im, c) for im in live_ims for c in live_cats]
    want_ev, want = _assert_equal(ev, res, gt, c2d, "sparse table", pairs=pairs)
    assert want["AP"] > 0 and (want_ev["recall"][0, :, 0] > 0).sum() >= 2


# ---- accumulation through the reused entry ---------------------------------------------------------------------------------------------------
def test_segment_of_scan_chunk_plus_one(engine):
    """category 1 holds COCO_ACC_CHUNK + 1 rows -- images of 300, the whole budget in one pair, plus the rest: sylph_coco_accumulate with one
    maxDet of 300 carries its counts and its precision maximum from chunk to chunk"""
    chunk = _lib.COCO_ACC_CHUNK
    n_full, rest = divmod(chunk + 1, 300)
    ims, cats = list(range(1, n_full + 3)), [1, 2]
    per = {im: 300 for im in ims[:n_full]}
    per[ims[n_full]] = rest
    gt, dets = lvis_case(21, ims, cats, gt_per_pair=lambda r, im, c: r.integers(2, 9) if c == 1 else 1,
                         det_per_pair=lambda r, im, c: per.get(im, 0) if c == 1 else (3 if im not in per else 0), federate=False)
    ev, res, _ = _run(engine, gt, dets, cats, "chunk + 1", batch=7)
    rows = torch.cat(ev._rows)
    assert int((rows[:, 6] == 0).sum()) == chunk + 1 and dets[1].shape[0] == 300


# ---- end to end: the query loops ---------------------------------------------------------------------------------------------------------------
class _Tee:
    """a DeviceLVISEvaluator that also keeps what detections_to_coco_rows makes of every batch, for the restatement"""

    def __init__(self, ev):
        self.ev, self.coco = ev, []

    def reset(self):
        self.ev.reset()
        self.coco = []

    def process(self, inputs, outputs):
        from sylph_amd.evaluation import detections_to_coco_rows
        self.ev.process(inputs, outputs)
        self.coco += detections_to_coco_rows(outputs, [x["image_id"] for x in inputs])

    def evaluate(self):
        return self.ev.evaluate()


@pytest.fixture(scope="module")
def query_model():
    from sylph_amd import synthetic as W
    from sylph_amd.runner import MetaFCOSRunner, create_cfg
    r = MetaFCOSRunner()
    cfg = create_cfg(r.get_default_cfg(), "sylph://LVISv1-Detection/Meta-FCOS/Meta-FCOS-finetune.yaml")
    assert cfg.MODEL.FCOS.POST_NMS_TOPK_TEST == 300
    model = r.build_model(cfg, dtype="bf16")
    model.load_state_dict(W.synthetic_state_dict(0, depth=50))
    model.eval()
    sizes = [(128, 160), (100, 150), (128, 160), (96, 128), (128, 128)]
    loader, batch = [], []
    for i, (h, w) in enumerate(sizes):
        batch.append({"image": W.synthetic_images(1, h, w, seed=30 + i)[0], "height": h + 20, "width": w + 10, "image_id": 100 + 7 * i})
        if len(batch) == 2 or i == len(sizes) - 1:
            loader.append(batch)
            batch = []
    return model, loader


def _made_up_gt(model, loader, code):
    """LVIS ground truth made from the model's own output: every third detection's box, rounded to half pixels, except those of one class
    per image; the detected classes with a box are positive, up to two others negative, one positive class not exhaustively annotated"""
    anns, images = [], []
    with torch.no_grad():
        for batch in loader:
            for x, out in zip(batch, model(batch, class_code=code, run_type="meta_learn_test_instance")):
                inst = out["instances"]
                assert len(inst) > 0, "the synthetic model detects something on every image"
                b, c = inst.pred_boxes.tensor.cpu().numpy().astype(np.float64), inst.pred_classes.cpu().numpy()
                skip, pos = len(images) % 5, set()
                for j in range(0, len(inst), 3):
                    if int(c[j]) == skip:
                        continue
                    x0, y0, x1, y1 = np.round(b[j] * 2) / 2
                    anns.append({"id": len(anns) + 1, "image_id": x["image_id"], "category_id": int(c[j]), "bbox": [x0, y0, max(x1 - x0, 1.0), max(y1 - y0, 1.0)],
                                 "area": float(max(x1 - x0, 1.0) * max(y1 - y0, 1.0)) * 0.8})
                    pos.add(int(c[j]))
                others = [k for k in range(5) if k not in pos]
                images.append({"id": x["image_id"], "neg_category_ids": others[:2], "not_exhaustive_category_ids": sorted(pos)[:1]})
    return {"images": images, "annotations": anns, "categories": [{"id": c, "name": f"class{c}", "frequency": "rcf"[c % 3]} for c in range(5)]}


def _assert_loop_result(tee, res, gt, what, positive=False):
    want_ev, want = LR.results(gt, tee.coco)
    for name in ("precision", "recall"):
        assert np.array_equal(_bits(getattr(tee.ev, name)), _bits(want_ev[name])), f"{what}: {name}"
    assert list(res["bbox"]) == list(want)
    for k in want:
        assert (math.isnan(res["bbox"][k]) and math.isnan(want[k])) or res["bbox"][k] == want[k], f"{what}: {k}"
    assert len(tee.coco) > 0 and (want["AP"] > 0 or not positive), f"{what}: the comparison is not vacuous"


def test_query_loops_end_to_end(query_model):
    from test_mixed_episodes_gpu import _code
    from sylph_amd.evaluation import (cache_query_dataset, inference_on_dataset_with_class_codes, inference_on_dataset_with_code_sets,
                                      release_query_records)
    from sylph_amd.lvis_eval import DeviceLVISEvaluator
    model, loader = query_model
    d0, d1 = _code("n5"), _code("n5b")
    gt = _made_up_gt(model, loader, d0)
    tee = _Tee(DeviceLVISEvaluator(gt, engine=model.engine))
    res = inference_on_dataset_with_class_codes(model, loader, tee, d0)
    _assert_loop_result(tee, res, gt, "class codes", positive=True)  # the ground truth was made from this run's boxes
    tees = [_Tee(DeviceLVISEvaluator(gt, engine=model.engine)) for _ in range(2)]
    out = inference_on_dataset_with_code_sets(model, loader, tees, [d0, d1])
    for g, (t, r) in enumerate(zip(tees, out)):
        _assert_loop_result(t, r, gt, f"code sets, set {g}", positive=g == 0)
    records = cache_query_dataset(model, loader)
    try:
        res = inference_on_dataset_with_class_codes(model, records, tee, d0)
        _assert_loop_result(tee, res, gt, "query records", positive=True)
    finally:
        release_query_records(records)
