"""COCO bbox evaluation on the GPU: DeviceCOCOEvaluator (coco_match_kernel + coco_accumulate_kernel behind two device sorts) against the
float64 numpy restatement tests/cocoeval_ref.py.

The criterion is BIT equality of precision [T, R, K, A, M], recall [T, K, A, M] and scores [T, R, K, A, M], and equal summary dicts with NaN at
the same keys: every operation on the way is one IEEE float64 add, multiply, divide or compare in a fixed order, so there is no tolerance.
The restatement sees detection_rows_to_coco of the very rows the evaluator holds.

Boxes lie on a half-pixel grid with widths that are multiples of 3 or 7, and detections are ground-truth boxes shifted by a third or a
seventh of their width among others: IoUs of exactly 0.5 and 0.75 and exact IoU ties occur.  Scores come from 8 fp32 values."""
import math

import numpy as np
import pytest
import torch

import cocoeval_ref as CR
from sylph_amd import _lib
from sylph_amd.evaluation import detection_rows_to_coco

pytestmark = pytest.mark.gpu
SIZES = [12, 14, 24, 28, 48, 56, 112, 120]  # 144 .. 784 small, 2304 / 3136 medium, 12544 / 14400 large
SCORES = np.array([0.0625 + 0.125 * i for i in range(8)], dtype=np.float32)


@pytest.fixture(scope="module")
def engine():
    from sylph_amd.engine import Engine
    eng = Engine(None, dtype="f32")
    yield eng
    eng.close()


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
def _gt_box(rng):
    w, h = float(rng.choice(SIZES)), float(rng.choice(SIZES))
    return [float(rng.integers(0, 400)) / 2, float(rng.integers(0, 400)) / 2, w, h]


def _near(rng, b):
    """a detection for ground-truth box b: the box itself, shifted by w / 3 (IoU 1/2) or w / 7 (IoU 3/4) where that is a whole number, shifted by
    half pixels, or resized"""
    x, y, w, h = b
    kind = int(rng.integers(0, 6))
    if kind == 1 and w % 3 == 0:
        x += w / 3 * (1 if rng.integers(0, 2) else -1)
    elif kind == 2 and w % 7 == 0:
        x += w / 7 * (1 if rng.integers(0, 2) else -1)
    elif kind == 3:
        x, y = x + float(rng.integers(-8, 9)) / 2, y + float(rng.integers(-8, 9)) / 2
    elif kind == 4:
        w, h = float(rng.choice(SIZES)), float(rng.choice(SIZES))
    elif kind == 5 and h % 3 == 0:
        y += h / 3
    return [x, y, x + w, y + h]


def make_case(seed, image_ids, cat_ids, gt_per_pair, det_per_pair, crowd=0.1, pair_fill=0.7):
    """-> (gt dict, {image id: (n, 6) fp32 rows x0 y0 x1 y1 score class}); class c is category cat_ids[c].  gt_per_pair / det_per_pair: callables
    (rng, image id, category id) -> count, or ints = the maximum of a uniform draw; a pair is empty on one side with probability 1 - pair_fill"""
    rng = np.random.default_rng(seed)
    anns, dets = [], {}
    count = lambda spec, im, c: int(spec(rng, im, c)) if callable(spec) else (int(rng.integers(1, spec + 1)) if rng.random() < pair_fill else 0)
    for im in image_ids:
        rows = []
        for k, c in enumerate(cat_ids):
            boxes = [_gt_box(rng) for _ in range(count(gt_per_pair, im, c))]
            for b in boxes:
                is_crowd = int(rng.random() < crowd)
                if is_crowd:
                    b[2], b[3] = 150.0, 120.0  # many detections fall inside
                area = b[2] * b[3] * float(rng.choice([1.0, 1.0, 0.75, 0.5, 0.3]))  # a segmentation's area: not w * h
                anns.append({"id": len(anns) + 1, "image_id": im, "category_id": c, "bbox": list(b), "area": area, "iscrowd": is_crowd})
            for _ in range(count(det_per_pair, im, c)):
                if boxes and rng.random() < 0.8:
                    box = _near(rng, boxes[int(rng.integers(0, len(boxes)))])
                else:
                    g = _gt_box(rng)
                    box = [g[0], g[1], g[0] + g[2], g[1] + g[3]]
                rows.append(box + [float(rng.choice(SCORES)), float(k)])
        order = rng.permutation(len(rows))
        dets[im] = np.array(rows, dtype=np.float32).reshape(-1, 6)[order]
    gt = {"images": [{"id": im} for im in image_ids], "annotations": [anns[i] for i in rng.permutation(len(anns))],
          "categories": [{"id": c, "name": f"cat{c}"} for c in cat_ids]}
    return gt, dets


def _outputs(rows, dev):
    from sylph_amd.structures import Boxes, Instances
    t = torch.from_numpy(rows).to(dev)
    return {"instances": Instances((300, 300), pred_boxes=Boxes(t[:, :4].contiguous()), scores=t[:, 4].contiguous(),
                                   pred_classes=t[:, 5].to(torch.int64))}


def _feed(ev, dets, order, batch):
    """process() over the images in `order`, `batch` at a time"""
    dev = torch.device("cuda", 0)
    ev.reset()
    for i in range(0, len(order), batch):
        ids = order[i:i + batch]
        ev.process([{"image_id": im} for im in ids], [_outputs(dets[im], dev) for im in ids])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _assert_equal(ev, res, gt, c2d, what, subsets=None, rows=None):
    rows = torch.cat(ev._rows) if rows is None else rows
    want_ev, want = CR.results(gt, detection_rows_to_coco(rows, c2d), ev.max_dets, subsets)
    for name in ("precision", "recall", "scores"):
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


def _run(engine, gt, dets, cat_ids, what, batch=7, seed=0, **kw):
    from sylph_amd.coco_eval import DeviceCOCOEvaluator
    c2d = {k: c for k, c in enumerate(cat_ids)}
    ev = DeviceCOCOEvaluator(gt, contiguous_to_dataset_id=c2d, engine=engine, **kw)
    order = [int(i) for i in np.random.default_rng(seed).permutation(sorted(dets))]
    _feed(ev, dets, order, batch)
    res = ev.evaluate()
    return ev, res, _assert_equal(ev, res, gt, c2d, what, kw.get("category_subsets"))


# ---- matching ------------------------------------------------------------------------------------------------------------------------------
def test_pairs_with_one_side_empty(engine):
    """D = 0 with G > 0 (counts into npig and nothing else), G = 0 with D > 0 (false positives, or ignored by their own area), and an image
    with neither"""
    ims, cats = [3, 5, 9, 11], [2, 4]
    gt, dets = make_case(1, ims, cats, gt_per_pair=lambda r, im, c: 3 if (im, c) in ((3, 2), (5, 4), (9, 2)) else 0,
                         det_per_pair=lambda r, im, c: 4 if (im, c) in ((3, 4), (5, 2), (9, 2)) else 0, crowd=0.0)
    ev, res, (want_ev, _) = _run(engine, gt, dets, cats, "one side empty", batch=1)
    assert dets[11].shape[0] == 0 and dets[3].shape[0] == 4
    assert (want_ev["recall"][:, :, 0, 2] >= 0).all(), "both categories have non-ignored ground truth"


@pytest.mark.parametrize("G", [1, 65, _lib.COCO_MATCH_TILE_GT, _lib.COCO_MATCH_TILE_GT + 1])
def test_ground_truth_count_of_a_pair(engine, G):
    """one box, more than a wave of boxes, the LDS tile bound and one past it (no tile: the IoU is recomputed, the flags live in scratch); a
    second, small pair rides along so that both paths run in the launch past the bound"""
    ims, cats = [1, 2], [1]
    gt, dets = make_case(10 + G, ims, cats, gt_per_pair=lambda r, im, c: G if im == 1 else 1,
                         det_per_pair=lambda r, im, c: 60 if im == 1 else 5, crowd=0.15)
    ev, res, (want_ev, want) = _run(engine, gt, dets, cats, f"G = {G}", batch=1)
    assert ev._tables(torch.device("cuda", 0))["max_per_pair"] == G
    assert want_ev["recall"][0, 0, 0, 2] > 0, "something matches"


@pytest.mark.parametrize("max_det,G", [(300, 100), (300, 55), (300, 56), (1024, 14)])
def test_tile_bound_shrunk_by_max_det(engine, max_det, G):
    """maxDets[-1] > 131 shrinks the LDS tile below COCO_MATCH_TILE_GT (55 boxes at 300, 13 at 1024): a pair between the shrunken bound
    and 128 takes the no-tile path and needs the scratch, which Engine.coco_match sizes from sylph_coco_match_tile_gt; the pair at the
    shrunken bound itself still uses the tile.  150 detections in the pair, so ranks past 100 count."""
    tile = _lib.lib().sylph_coco_match_tile_gt(max_det)
    assert tile < _lib.COCO_MATCH_TILE_GT and (G <= _lib.COCO_MATCH_TILE_GT) and G in (tile, tile + 1, 100)
    ims, cats = [1, 2], [1]
    gt, dets = make_case(300 + G, ims, cats, gt_per_pair=lambda r, im, c: G if im == 1 else 1,
                         det_per_pair=lambda r, im, c: 150 if im == 1 else 5, crowd=0.15)
    ev, res, (want_ev, _) = _run(engine, gt, dets, cats, f"max_det {max_det}, G = {G}", batch=1, max_dets=(1, 10, max_det))
    assert want_ev["recall"][0, 0, 0, 2] > 0, "something matches"


def test_match_without_scratch_is_refused_before_any_launch(engine):
    """the C entry with a NULL scratch and a pair past the bound of its max_det fails by name on the host: nothing is launched"""
    from ctypes import c_void_p
    from sylph_amd.engine import _ptr
    dev = torch.device("cuda", 0)
    z = lambda *shape, dt=torch.float64: torch.zeros(*shape, dtype=dt, device=dev)
    off, thr, rng = z(2, dt=torch.int32), z(10), z(4, 2)
    box, area, crowd, npig = z(100, 4), z(100), z(100, dt=torch.int32), z(1, 4, dt=torch.int32)
    for max_det, max_gt in ((300, 56), (100, 129)):
        rc = engine.L.sylph_coco_match(engine._ctx, 0, c_void_p(0), 1, 1, _ptr(off), _ptr(box), _ptr(area), _ptr(crowd), _ptr(off), max_gt, 10,
                                       _ptr(thr), 4, _ptr(rng), max_det, c_void_p(0), c_void_p(0), c_void_p(0), _ptr(npig))
        assert rc != 0 and b"gt_scratch_dev" in engine.L.sylph_last_error() and b"sylph_coco_match_tile_gt" in engine.L.sylph_last_error()
    rc = engine.L.sylph_coco_match(engine._ctx, 0, c_void_p(0), 1, 1, _ptr(off), _ptr(box), _ptr(area), _ptr(crowd), _ptr(off), 55, 10,
                                   _ptr(thr), 4, _ptr(rng), 300, c_void_p(0), c_void_p(0), c_void_p(0), _ptr(npig))
    assert rc == 0, engine.L.sylph_last_error()  # at the bound no scratch is needed (an empty pair table: the one block returns at once)
    torch.cuda.synchronize()


def test_distributed_flag_on_one_rank(engine):
    """distributed=True without a process group: _gather falls through and the result is the single-process one"""
    ims, cats = [3, 5, 9], [2, 4]
    gt, dets = make_case(8, ims, cats, gt_per_pair=3, det_per_pair=6)
    _run(engine, gt, dets, cats, "distributed, one rank", batch=2, distributed=True)


def test_one_more_detection_than_max_dets(engine):
    """D = maxDets[-1] + 1: the lowest-scored row of the pair (the last to arrive among the lowest) is cut, and its rank excludes it everywhere"""
    ims, cats = [4, 6], [7, 8]
    gt, dets = make_case(5, ims, cats, gt_per_pair=lambda r, im, c: 6, det_per_pair=lambda r, im, c: 101 if (im, c) == (4, 7) else 9)
    ev, res, _ = _run(engine, gt, dets, cats, "D = 101", batch=7)
    small = _run(engine, gt, dets, cats, "maxDets (1, 2, 5)", batch=1, max_dets=(1, 2, 5))[1]["bbox"]
    assert "AR@5" in small and "AR@100" not in small


# ---- the seeded random set --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_set():
    ims, cats = [10 + 3 * i for i in range(40)], [1, 3, 4, 7, 20, 90]
    rng = np.random.default_rng(99)
    empty = {int(i) for i in rng.choice(ims, 3, replace=False)}
    # category 90: crowd-only or absent ground truth (npig = 0) but detections
    gt, dets = make_case(7, ims, cats, gt_per_pair=lambda r, im, c: 0 if im in empty or c == 90 or r.random() < 0.25 else r.integers(1, 6),
                         det_per_pair=lambda r, im, c: 0 if im in empty or r.random() < 0.2 else r.integers(1, 14), crowd=0.12)
    n = len(gt["annotations"])
    gt["annotations"] += [{"id": n + 1 + j, "image_id": ims[j], "category_id": 90, "bbox": [10.0, 10.0, 150.0, 120.0], "area": 9000.0, "iscrowd": 1}
                          for j in range(5)]
    return ims, cats, gt, dets


@pytest.mark.parametrize("batch", [1, 7])
def test_random_set_shuffled(engine, random_set, batch):
    ims, cats, gt, dets = random_set
    ev, res, (want_ev, want) = _run(engine, gt, dets, cats, f"random set, batches of {batch}", batch=batch, seed=batch)
    assert any(a["iscrowd"] for a in gt["annotations"]) and any(a["area"] != a["bbox"][2] * a["bbox"][3] for a in gt["annotations"])
    rows = torch.cat(ev._rows).cpu().numpy()
    assert len(np.unique(rows[:, 5])) == 8, "eight score values: ties everywhere"
    k90 = cats.index(90)
    assert np.all(want_ev["precision"][:, :, k90] == -1) and math.isnan(want["AP-cat90"]), "category 90 has no non-ignored ground truth"
    assert 0 < want["AP"] < 100 and 0 < want["AP75"] < want["AP50"] and want["AR@1"] < want["AR@10"]
    ious = [CR.iou([r[0], r[1], float(r[2]) - float(r[0]), float(r[3]) - float(r[1])], a["bbox"], False)
            for im in ims[:10] for r in dets[im].tolist() for a in gt["annotations"] if a["image_id"] == im and not a["iscrowd"]]
    assert 0.5 in ious and 0.75 in ious, "IoUs exactly at a threshold occur"


def test_category_subsets(engine, random_set):
    ims, cats, gt, dets = random_set
    subsets = {"novel": [3, 20, 90], "base": [1, 4, 7]}
    ev, res, (_, want) = _run(engine, gt, dets, cats, "subsets", category_subsets=subsets)
    assert all(k in res["bbox"] for k in ("nAP", "nAP50", "nAR@100", "bAP", "bARl")) and res["bbox"]["nAP"] != res["bbox"]["bAP"]


def test_padding_rows_in_the_middle(engine, random_set):
    """gather_detection_rows pads every rank's block with valid = 0 rows: two blocks, the first half full"""
    from sylph_amd.coco_eval import DeviceCOCOEvaluator
    from sylph_amd.evaluation import gather_detection_rows
    ims, cats, gt, dets = random_set
    c2d = {k: c for k, c in enumerate(cats)}
    ev = DeviceCOCOEvaluator(gt, contiguous_to_dataset_id=c2d, engine=engine)
    _feed(ev, dets, ims[::-1], 7)
    rows = torch.cat(ev._rows)
    half = rows.shape[0] // 2
    blocks = [gather_detection_rows(rows[:half], half + 300), gather_detection_rows(rows[half:], half + 300)]
    assert float(blocks[0][half:, 7].sum()) == 0 and blocks[0].shape[0] == half + 300
    ev._rows = blocks
    _assert_equal(ev, ev.evaluate(), gt, c2d, "padding rows", rows=rows)


# ---- accumulation ----------------------------------------------------------------------------------------------------------------------------
def test_segment_of_scan_chunk_plus_one(engine):
    """category 1 holds COCO_ACC_CHUNK + 1 rows (ten pairs of 100, one of 25): the counts and the precision maximum are carried from chunk to
    chunk; with maxDets (1, 10, 100) two of the three cells also skip most rows of the segment"""
    chunk = _lib.COCO_ACC_CHUNK
    ims, cats = list(range(1, 13)), [1, 2]
    n_full, rest = divmod(chunk + 1, 100)
    per = {im: 100 for im in ims[:n_full]}
    per[ims[n_full]] = rest
    gt, dets = make_case(21, ims, cats, gt_per_pair=lambda r, im, c: r.integers(2, 9) if c == 1 else 1,
                         det_per_pair=lambda r, im, c: per.get(im, 0) if c == 1 else 3)
    ev, res, _ = _run(engine, gt, dets, cats, "chunk + 1", batch=7)
    rows = torch.cat(ev._rows)
    assert int((rows[:, 6] == 0).sum()) == chunk + 1


def test_evaluator_with_its_own_engine_and_refusals(random_set):
    from sylph_amd.coco_eval import DeviceCOCOEvaluator
    ims, cats, gt, dets = random_set
    c2d = {k: c for k, c in enumerate(cats)}
    ev = DeviceCOCOEvaluator(gt, contiguous_to_dataset_id=c2d)
    _feed(ev, dets, ims[:6], 2)
    _assert_equal(ev, ev.evaluate(), gt, c2d, "own engine")
    ev.reset()
    assert ev.evaluate()["bbox"]["AP"] == 0.0  # no detections at all: recall 0, precision 0 wherever there is ground truth
    bad = dict(dets)
    bad[5] = dets[ims[0]]
    _feed(ev, bad, [ims[1], 5], 2)
    with pytest.raises(ValueError, match="image id 5"):
        ev.evaluate()
    with pytest.raises(RuntimeError, match="COCO_MATCH_MAX_DETS"):
        big = DeviceCOCOEvaluator(gt, contiguous_to_dataset_id=c2d, max_dets=(1, 10, 2000), engine=ev.engine)
        _feed(big, dets, ims[:2], 2)
        big.evaluate()
    ev.engine.close()


# ---- end to end: the query loops ---------------------------------------------------------------------------------------------------------------
class _Tee:
    """a DeviceCOCOEvaluator that also keeps what detections_to_coco_rows makes of every batch, for the restatement"""

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
    cfg = create_cfg(r.get_default_cfg(), "sylph://COCO-Detection/Meta-FCOS/Meta-FCOS-finetune.yaml")
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
    """ground truth made from the model's own output: every third detection's box, rounded to half pixels, plus a crowd box per image"""
    anns, images = [], []
    with torch.no_grad():
        for batch in loader:
            for x, out in zip(batch, model(batch, class_code=code, run_type="meta_learn_test_instance")):
                images.append({"id": x["image_id"]})
                inst = out["instances"]
                assert len(inst) > 0, "the synthetic model detects something on every image"
                b, c = inst.pred_boxes.tensor.cpu().numpy().astype(np.float64), inst.pred_classes.cpu().numpy()
                for j in range(0, len(inst), 3):
                    x0, y0, x1, y1 = np.round(b[j] * 2) / 2
                    anns.append({"id": len(anns) + 1, "image_id": x["image_id"], "category_id": int(c[j]), "bbox": [x0, y0, max(x1 - x0, 1.0), max(y1 - y0, 1.0)],
                                 "area": float(max(x1 - x0, 1.0) * max(y1 - y0, 1.0)) * 0.8, "iscrowd": 0})
                anns.append({"id": len(anns) + 1, "image_id": x["image_id"], "category_id": 0, "bbox": [0.0, 0.0, 60.0, 60.0], "area": 3600.0, "iscrowd": 1})
    return {"images": images, "annotations": anns, "categories": [{"id": c, "name": f"class{c}"} for c in range(5)]}


def _assert_loop_result(tee, res, gt, what, positive=False):
    want_ev, want = CR.results(gt, tee.coco)
    for name in ("precision", "recall", "scores"):
        assert np.array_equal(_bits(getattr(tee.ev, name)), _bits(want_ev[name])), f"{what}: {name}"
    assert list(res["bbox"]) == list(want)
    for k in want:
        assert (math.isnan(res["bbox"][k]) and math.isnan(want[k])) or res["bbox"][k] == want[k], f"{what}: {k}"
    assert len(tee.coco) > 0 and (want["AP"] > 0 or not positive), f"{what}: the comparison is not vacuous"


def test_query_loops_end_to_end(query_model):
    from test_mixed_episodes_gpu import _code
    from sylph_amd.coco_eval import DeviceCOCOEvaluator
    from sylph_amd.evaluation import (cache_query_dataset, inference_on_dataset_with_class_codes, inference_on_dataset_with_code_sets,
                                      release_query_records)
    model, loader = query_model
    d0, d1 = _code("n5"), _code("n5b")
    gt = _made_up_gt(model, loader, d0)
    tee = _Tee(DeviceCOCOEvaluator(gt, engine=model.engine))
    res = inference_on_dataset_with_class_codes(model, loader, tee, d0)
    _assert_loop_result(tee, res, gt, "class codes", positive=True)  # the ground truth was made from this run's boxes
    tees = [_Tee(DeviceCOCOEvaluator(gt, engine=model.engine)) for _ in range(2)]
    out = inference_on_dataset_with_code_sets(model, loader, tees, [d0, d1])
    for g, (t, r) in enumerate(zip(tees, out)):
        _assert_loop_result(t, r, gt, f"code sets, set {g}", positive=g == 0)
    records = cache_query_dataset(model, loader)
    try:
        res = inference_on_dataset_with_class_codes(model, records, tee, d0)
        _assert_loop_result(tee, res, gt, "query records", positive=True)
    finally:
        release_query_records(records)
