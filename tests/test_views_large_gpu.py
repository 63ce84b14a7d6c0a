"""The large view merge on the GPU (sylph_merge_views_large, Engine.merge_views_large, the model's route to it): against the one-block
merge where both accept the pool, against the greedy numpy reference (tests/views_large_ref.py) above its capacity, and end to end
against the composition of the existing paths.  Every comparison is exact.  The rows come from views_ref.draw_rows, which enforces
and asserts a 1e-4 IoU margin from NMS_TH on the CPU; the one hand-made pool (disjoint boxes and exact copies) has IoUs of 0 and 1."""
import ctypes

import numpy as np
import pytest
import torch

import views_large_ref as LR
import views_ref as VR
from test_views_cpu import MERGE_COUNTS, interleaved_table
from test_views_gpu import _assert_merged, _assert_model, _codes, _composition, _engine, _model, _rows, _u8
from test_views_large_cpu import drawn_pool, one_source_table, pool_4300

pytestmark = pytest.mark.gpu

THR = 0.6
# the tile and chunk constants of csrc/merge_views_large.hip (csrc/kernels.h; DESIGN lists them)
SORT_TILE, CHUNK, KEPT_LDS = 2048, 64, 2048


@pytest.fixture(scope="module")
def sd():
    from sylph_amd import synthetic as W
    return W.synthetic_state_dict(0, depth=50)


@pytest.fixture(scope="module")
def eng():
    e = _engine("bf16", None, **{"MODEL.FCOS.NMS_TH": THR, "MODEL.FCOS.POST_NMS_TOPK_TEST": 100})
    yield e
    e.close()


def _prefix(pool, n_views):
    table, boxes, scores, classes, counts = pool
    return table[:n_views], boxes[:n_views], scores[:n_views], classes[:n_views], counts[:n_views]


def _check(eng, pool, n_src, topk, what, thr=THR, work=True, max_out=None):
    """merge_views_large against the numpy reference; work: NMS must drop rows and rule 5 must cut (K > 0)"""
    table, boxes, scores, classes, counts = pool
    K = int(eng.sc.post_nms_topk) if topk is None else topk
    want = LR.merge_large_ref(table, boxes, scores, classes, counts, n_src, thr, K)
    if work:
        rows = sum(min(max(int(c), 0), scores.shape[1]) for c in counts)
        assert sum(w["kept"] for w in want) < rows, f"{what}: NMS has no work"
        if K > 0:
            assert max(w["kept"] for w in want) > K, f"{what}: rule 5 has no work at K = {K}"
    if max_out is None:
        max_out = max(len(w["scores"]) for w in want) + 3
    got = eng.merge_views_large(table, _rows(boxes, scores, classes, counts), max_out=max_out, n_src=n_src, topk=topk)
    _assert_merged(got, want, what)
    return got, want


def _same(a, b):
    return all(torch.equal(x[k], y[k]) for x, y in zip(a, b) for k in ("pred_boxes", "scores", "pred_classes", "view_index", "view_row"))


# ------------------------------------------------------------------------------------------------ 1: equals the one-block merge
def _old_kernel_pools():
    table = interleaved_table()
    small = (table,) + VR.draw_rows(table, 16, MERGE_COUNTS, 3, seed=11, thr=THR, score_levels=12)
    t1280 = [{"source": 0, "crop": (3 * (v % 5), 2 * (v % 3), 250, 200), "flip": v % 2 == 1} for v in range(20)]
    t1280.insert(7, {"source": 1, "crop": (0, 0, 250, 200), "flip": False})
    c1280 = [64] * 21
    c1280[7] = 3
    mid = (t1280,) + VR.draw_rows(t1280, 64, c1280, 4, seed=5, thr=THR, score_levels=0, n_objects=60)
    return {"interleaved": (small, 3), "1280 rows": (mid, 2), "4096 rows": (drawn_pool(64, 64, 5, 9, 30), 1)}


@pytest.fixture(scope="module")
def old_kernel_pools():
    return _old_kernel_pools()


@pytest.mark.parametrize("thr", [0.6, 0.0])
@pytest.mark.parametrize("K", [100, 7, 0])
def test_equals_the_block_merge(old_kernel_pools, thr, K):
    e = _engine("bf16", None, **{"MODEL.FCOS.NMS_TH": thr, "MODEL.FCOS.POST_NMS_TOPK_TEST": K})
    for name, (pool, n_src) in old_kernel_pools.items():
        table, boxes, scores, classes, counts = pool
        want = LR.merge_large_ref(table, boxes, scores, classes, counts, n_src, thr, K)
        total = int(np.sum(counts))
        if thr > 0:
            assert sum(w["kept"] for w in want) < total, f"{name}: NMS has no work"
        if K == 7 or (K == 100 and total >= 1280):
            assert max(w["kept"] for w in want) > K, f"{name}: rule 5 has no work at K = {K}"
        old = e.merge_views(table, _rows(boxes, scores, classes, counts), max_out=total, n_src=n_src)
        new = e.merge_views_large(table, _rows(boxes, scores, classes, counts), max_out=total, n_src=n_src)
        assert [o["scores"].numel() for o in old] == [n["scores"].numel() for n in new], f"{name}: counts"
        assert _same(old, new), f"{name}, NMS_TH {thr}, K {K}: the two merges differ"
        _assert_merged(new, want, f"{name}, NMS_TH {thr}, K {K}")
    e.close()


# ------------------------------------------------------------------------------------------------ 2: above the capacity, against numpy
def test_4160_rows_the_block_merge_refuses(eng):
    pool = drawn_pool(65, 64, 5, 13)
    with pytest.raises(RuntimeError, match="MERGE_POOL_CAP"):
        eng.merge_views(pool[0], _rows(*pool[1:]))
    _check(eng, pool, 1, None, "65 x 64 rows")


def test_4300_rows_with_tied_scores(eng):
    got, want = _check(eng, pool_4300(), 1, 100, "4300 rows, K 100")
    assert len(want[0]["scores"]) > 100, "the ties of the 100th place are kept"


@pytest.fixture(scope="module")
def pool_15000():
    """150 views x 100 rows over three interleaved sources; source 3 has no view, source 4 two empty views, source 5 one row"""
    table, boxes, scores, classes, counts = drawn_pool(150, 100, 5, 3, 0, 60, 3)
    extra = [{"source": 4, "crop": (0, 0, 250, 200), "flip": False}, {"source": 5, "crop": (5, 4, 250, 200), "flip": True},
             {"source": 4, "crop": (2, 2, 250, 200), "flip": True}]
    eb, es, ec, en = VR.draw_rows(extra, 100, [0, 1, 0], 5, seed=4, thr=THR)
    table = table[:70] + extra[:2] + table[70:] + extra[2:]  # the extra views sit among the others
    cat = lambda a, b: np.concatenate([a[:70], b[:2], a[70:], b[2:]])
    return table, cat(boxes, eb), cat(scores, es), cat(classes, ec), cat(counts, en)


def test_15000_rows_of_three_sources_and_empty_ones(eng, pool_15000):
    got, want = _check(eng, pool_15000, 6, 100, "15000 rows")
    assert [len(w["scores"]) for w in want][3:] == [0, 0, 1]
    # 7: the same call again gives the same bits
    again = eng.merge_views_large(pool_15000[0], _rows(*pool_15000[1:]), max_out=max(len(w["scores"]) for w in want) + 3, n_src=6, topk=100)
    assert _same(got, again)


# ------------------------------------------------------------------------------------------------ 3: class layout
@pytest.fixture(scope="module")
def one_class_pool():
    return drawn_pool(6000, 1, 1, 5)  # 6000 views of one row: every prefix is a pool of its own


def test_one_class_is_one_long_segment(eng, one_class_pool):
    _check(eng, one_class_pool, 1, 100, "6000 rows of one class")
    _check(eng, one_class_pool, 1, 0, "6000 rows of one class, K 0")


def test_1203_classes_are_many_short_segments(eng):
    pool = drawn_pool(60, 100, 1203, 6)
    assert len(np.unique(pool[3])) > 500  # (four rows in five take the class of one of the 60 objects)
    _check(eng, pool, 1, 100, "6000 rows of 1203 classes")


def test_class_ids_are_any_int32(eng):
    table, boxes, scores, classes, counts = drawn_pool(43, 100, 4, 17)
    ids = np.array([0, 7, 65536, 2 ** 31 - 1], dtype=np.int32)
    got, _ = _check(eng, (table, boxes, scores, ids[classes], counts), 1, 100, "class ids up to 2^31 - 1")
    assert set(got[0]["pred_classes"].tolist()) <= set(ids.tolist()) and int(got[0]["pred_classes"].max()) == 2 ** 31 - 1


# ------------------------------------------------------------------------------------------------ 4: rule 5, truncation
def test_topk_values_and_truncation(eng):
    pool = pool_4300()
    kept = LR.merge_large_ref(*pool, 1, THR, 0)[0]["kept"]
    assert 100 < kept < 4300
    _check(eng, pool, 1, 0, "topk 0", max_out=kept)  # max_out exactly the kept count: not truncated
    for topk in (1, 100, kept + 50):
        _check(eng, pool, 1, topk, f"topk {topk}", work=topk < kept)
    _check(eng, pool, 1, None, "topk None is POST_NMS_TOPK_TEST")
    with pytest.raises(RuntimeError, match="max_out"):
        eng.merge_views_large(pool[0], _rows(*pool[1:]), max_out=kept - 1, topk=0)
    _check(eng, pool, 1, 0, "after a truncated call")


def test_a_truncated_source_holds_its_first_rows(eng):
    """the C entry: status bit 1 and the first max_out rows in order"""
    from sylph_amd.engine import _iarr, _ptr
    table, boxes, scores, classes, counts = pool_4300()
    want = LR.merge_large_ref(table, boxes, scores, classes, counts, 1, THR, 0, max_out=64)[0]
    assert want["truncated"]
    nv, max_in, max_out = len(table), 100, 64
    r = _rows(boxes, scores, classes, counts)
    fa = lambda k: (ctypes.c_float * nv)(*[float(t["crop"][k]) for t in table])
    ob, osc = torch.zeros(max_out, 4, device="cuda"), torch.zeros(max_out, device="cuda")
    oi = torch.zeros(3, max_out, device="cuda", dtype=torch.int32)
    tail = torch.full((2,), -1, device="cuda", dtype=torch.int32)
    need = eng.L.sylph_merge_views_large_bytes(1, nv, max_in)
    ws = torch.empty(need, device="cuda", dtype=torch.uint8)
    rc = eng.L.sylph_merge_views_large(eng._ctx, 1, nv, _iarr([0] * nv), fa(0), fa(1), fa(2), _iarr([1 if t["flip"] else 0 for t in table]), max_in,
                                       _ptr(r["boxes"]), _ptr(r["scores"]), _ptr(r["classes"]), _ptr(r["counts"]), 0, max_out, _ptr(ob), _ptr(osc),
                                       _ptr(oi[0]), _ptr(oi[1]), _ptr(oi[2]), _ptr(tail), ctypes.c_void_p(tail.data_ptr() + 4), _ptr(ws), need)
    assert rc == 0, eng.L.sylph_last_error()
    assert tail.tolist() == [64, 2]
    assert torch.equal(ob.cpu(), torch.from_numpy(want["pred_boxes"])) and torch.equal(osc.cpu(), torch.from_numpy(want["scores"]))
    assert torch.equal(oi[1].cpu().long(), torch.from_numpy(want["view_index"])) and torch.equal(oi[2].cpu().long(), torch.from_numpy(want["view_row"]))


# ------------------------------------------------------------------------------------------------ 5: counts outside [0, max_in]
def test_counts_outside_the_rows_are_clamped(eng):
    table, boxes, scores, classes, counts = pool_4300()
    wild, clamped = counts.copy(), counts.copy()
    wild[0], wild[5], wild[42] = 100 + 1, -1, 2 ** 31 - 1
    clamped[5] = 0
    want = LR.merge_large_ref(table, boxes, scores, classes, clamped, 1, THR, 100)
    got = eng.merge_views_large(table, _rows(boxes, scores, classes, wild), max_out=400, topk=100)
    _assert_merged(got, want, "clamped counts")


# ------------------------------------------------------------------------------------------------ 6: boundaries
@pytest.fixture(scope="module")
def rows_8193():
    return drawn_pool(8193, 1, 8, 8, 0, 200)  # 8193 views of one row, 8 classes


@pytest.mark.parametrize("n", [SORT_TILE - 1, SORT_TILE, SORT_TILE + 1, 4097, 8191, 8192, 8193])
def test_pool_sizes_around_the_sorted_lengths(eng, rows_8193, n):
    _check(eng, _prefix(rows_8193, n), 1, 100, f"{n} rows")


def test_16385_rows_cross_the_next_power_of_two(eng, rows_8193):
    """source 0 holds the 8193 rows, source 1 its first 8192 again (a source's rows meet no other source's)"""
    table, boxes, scores, classes, counts = rows_8193
    second = [dict(t, source=1) for t in table[:8192]]
    pool = (table + second, np.concatenate([boxes, boxes[:8192]]), np.concatenate([scores, scores[:8192]]),
            np.concatenate([classes, classes[:8192]]), np.concatenate([counts, counts[:8192]]))
    got, _ = _check(eng, pool, 2, 100, "16385 rows")
    assert got[0]["scores"].numel() > 0 and got[1]["scores"].numel() > 0


@pytest.mark.parametrize("n", [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK + 1])
def test_single_class_segments_around_the_chunk(eng, one_class_pool, n):
    _check(eng, _prefix(one_class_pool, n), 1, 7, f"one class, {n} rows", work=n >= CHUNK - 1)


@pytest.mark.parametrize("n_kept", [KEPT_LDS - 1, KEPT_LDS, KEPT_LDS + 1, KEPT_LDS + 70])
def test_kept_boxes_around_the_lds_list(eng, n_kept):
    """One class, n_kept disjoint boxes and 40 exact copies with lower scores: the copies of the last boxes are suppressed by kept
    boxes that lie beyond the LDS list when n_kept passes MERGE_LARGE_KEPT_LDS.  IoUs are 0 or 1: the margin is 0.4."""
    max_in = 100
    rng = np.random.RandomState(n_kept)
    n = n_kept + 40
    nv = (n + max_in - 1) // max_in
    table = one_source_table(nv)
    cell = np.arange(n_kept)
    src_box = np.stack([20.0 + 8 * (cell % 64), 10.0 + 8 * (cell // 64), 25.0 + 8 * (cell % 64), 15.0 + 8 * (cell // 64)], axis=1)
    copies = np.concatenate([np.arange(n_kept - 20, n_kept), rng.choice(n_kept - 20, 20, replace=False)])
    src_box = np.concatenate([src_box, src_box[copies]]).astype(np.float32)
    sc = np.concatenate([np.linspace(0.99, 0.5, n_kept), np.linspace(0.4, 0.3, 40)]).astype(np.float32)
    order = rng.permutation(n)  # which row of the buffers a box lands in
    boxes, scores = np.zeros((nv, max_in, 4), np.float32), np.zeros((nv, max_in), np.float32)
    counts = np.array([min(max_in, n - v * max_in) for v in range(nv)], dtype=np.int32)
    for k, slot in enumerate(order):
        v, r = divmod(int(slot), max_in)
        x0, y0, cw = table[v]["crop"][:3]
        b = src_box[k] - np.array([x0, y0, x0, y0], np.float32)
        if table[v]["flip"]:
            b = np.array([cw - b[2], b[1], cw - b[0], b[3]], np.float32)
        boxes[v, r], scores[v, r] = b, sc[k]
    for v in range(nv):  # rows of a view in descending score order, as decode leaves them
        o = np.argsort(-scores[v, :counts[v]], kind="stable")
        boxes[v, :counts[v]], scores[v, :counts[v]] = boxes[v, o], scores[v, o]
    classes = np.full((nv, max_in), 3, np.int32)
    assert VR.min_iou_margin(table, boxes, scores, classes, counts, 1, THR) >= 0.39
    got, want = _check(eng, (table, boxes, scores, classes, counts), 1, 0, f"{n_kept} kept boxes")
    assert want[0]["kept"] == n_kept


# ------------------------------------------------------------------------------------------------ 8: the model, end to end
def _big_source():
    from sylph_amd.views import tile_views
    src = _u8(330, 440, 51)
    views = tile_views(330, 440, (96, 96), 0.25, 64, 160)
    assert len(views) == 31 and {v["size"] for v in views} == {(64, 64), (64, 85)}
    return src, views


def _composition_with_work(model, srcs, views, codes, K, monkeypatch):
    """_composition with rule 5's K for its numpy merge (the engine took its copy of the config when it was made, so only that merge
    sees K), after asserting on the very rows it merges that NMS drops some and that more than K stay -> merged, kept rows per source"""
    seen = {}
    real = VR.merge_ref

    def spy(table, boxes, scores, classes, counts, n_src, thr, k):
        seen["kept"] = [w["kept"] for w in LR.merge_large_ref(table, boxes, scores, classes, counts, n_src, thr, 0)]
        seen["rows"] = int(counts.sum())
        return real(table, boxes, scores, classes, counts, n_src, thr, k)

    monkeypatch.setattr(VR, "merge_ref", spy)
    monkeypatch.setattr(model.cfg.MODEL.FCOS, "POST_NMS_TOPK_TEST", K)
    want = _composition(model, srcs, views, codes)
    monkeypatch.undo()
    assert sum(seen["kept"]) < seen["rows"], "NMS has no work"
    assert max(seen["kept"]) > K, f"rule 5 has no work at K = {K}: {seen['kept']} rows kept"
    return want, seen["kept"]


def test_model_31_views_equal_the_composition(sd, monkeypatch):
    model = _model("bf16", sd)
    src, views = _big_source()
    assert len(views) * model.engine.default_max_out() == 6200
    d0 = _codes(5, 42)
    batch = [{"image_u8": torch.from_numpy(src), "resize_hw": (96, 128), "views": views}]
    got = model(batch, class_code=d0, run_type="meta_learn_test_instance")
    want, _ = _composition_with_work(model, [src], [views], d0, int(model.cfg.MODEL.FCOS.POST_NMS_TOPK_TEST), monkeypatch)
    _assert_model(got, want, [src])


def test_model_max_detections_is_the_merge_keep_count(sd, monkeypatch):
    """ "max_detections": rule 5's K of the merged result only, in 2 K output rows; also as SylphPredictor hands it over"""
    from sylph_amd.predictor import SylphPredictor
    model = _model("bf16", sd)
    src, views = _big_source()
    d0 = _codes(5, 42)
    kw = dict(class_code=d0, run_type="meta_learn_test_instance")
    batch = [{"image_u8": torch.from_numpy(src), "resize_hw": (96, 128), "views": views}]
    default = model(batch, **kw)
    got = model([dict(batch[0], max_detections=300)], **kw)
    want, kept = _composition_with_work(model, [src], [views], d0, 300, monkeypatch)
    _assert_model(got, want, [src])
    assert len(got[0]["instances"]) >= 300 > len(default[0]["instances"]), "the K of the inputs replaced the config's"
    # a K above max_out / 2 of the default (200 rows): the output buffers follow K
    many = model([dict(batch[0], max_detections=kept[0] + 10)], **kw)
    assert len(many[0]["instances"]) == kept[0]
    # the predictor's input dict (its constructor needs a checkpoint and class codes on disk: only _preprocess runs here)
    pred = SylphPredictor.__new__(SylphPredictor)
    pred.min_size, pred.max_size, pred.fused_preprocess, pred.input_format, pred._pinned = 64, 160, True, "BGR", {}
    pred.tiles, pred.tile_overlap, pred.max_detections = (96, 96), 0.25, 300
    inputs = pred._preprocess(src)
    assert inputs["max_detections"] == 300 and inputs["views"] == views
    _assert_model(model([inputs], **kw), want, [src])
    pred.max_detections = None
    assert "max_detections" not in pred._preprocess(src)


def test_model_batch_of_a_large_and_a_small_source(sd, monkeypatch):
    from sylph_amd.views import tile_views
    model = _model("bf16", sd)
    src, views = _big_source()
    small = _u8(150, 200, 41)
    small_views = tile_views(150, 200, (96, 96), 0.25, 96, 160)
    assert len(small_views) == 7
    d0 = _codes(5, 42)
    kw = dict(class_code=d0, run_type="meta_learn_test_instance")
    batch = [{"image_u8": torch.from_numpy(src), "resize_hw": (96, 128), "views": views},
             {"image_u8": torch.from_numpy(small), "resize_hw": (96, 128), "views": small_views}]
    got = model(batch, **kw)
    want, _ = _composition_with_work(model, [src, small], [views, small_views], d0, int(model.cfg.MODEL.FCOS.POST_NMS_TOPK_TEST), monkeypatch)
    _assert_model(got, want, [src, small])
    with pytest.raises(ValueError, match="max_detections"):
        model([dict(batch[0], max_detections=300), batch[1]], **kw)
    with pytest.raises(ValueError, match="max_detections"):  # no views, no merge: refused, not ignored
        model([{"image_u8": torch.from_numpy(small), "resize_hw": (96, 128), "max_detections": 300}], **kw)


# ------------------------------------------------------------------------------------------------ 9: refusals by name
def test_refusals_by_name(eng):
    from sylph_amd.engine import _iarr, _ptr
    z = lambda *s, dt=torch.float32: torch.zeros(*s, device="cuda", dtype=dt)
    max_out = 8
    outs = [torch.full((max_out * 4,), -7.0, device="cuda"), torch.full((max_out,), -7.0, device="cuda")] + \
           [torch.full((max_out,), -7, device="cuda", dtype=torch.int32) for _ in range(5)]

    def call(nv, max_in, ws, ws_bytes, bufs):
        fa = (ctypes.c_float * nv)(*([0.0] * nv))
        return eng.L.sylph_merge_views_large(eng._ctx, 1, nv, _iarr([0] * nv), fa, fa, fa, _iarr([0] * nv), max_in, *[_ptr(b) for b in bufs], -1,
                                             max_out, *[_ptr(t) for t in outs[:6]], _ptr(outs[6]), ws, ws_bytes)

    dummy = [z(16), z(16), z(16, dt=torch.int32), z(16, dt=torch.int32)]  # a host check: the buffers are never read
    some = z(64, dt=torch.uint8)
    assert call(5243, 200, _ptr(some), 64, dummy) != 0 and b"MERGE_LARGE_POOL_CAP" in eng.L.sylph_last_error()  # 1 048 600 rows
    nv, max_in = 30, 200
    bufs = [z(nv, max_in, 4), z(nv, max_in), z(nv, max_in, dt=torch.int32), z(nv, dt=torch.int32)]
    need = eng.L.sylph_merge_views_large_bytes(1, nv, max_in)
    assert need > 0
    assert call(nv, max_in, None, need, bufs) != 0 and b"workspace is NULL" in eng.L.sylph_last_error()
    ws = z(need, dt=torch.uint8)
    assert call(nv, max_in, _ptr(ws), need - 1, bufs) != 0 and b"sylph_merge_views_large_bytes asks for" in eng.L.sylph_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in outs), "a refused call writes nothing"
    assert call(nv, max_in, _ptr(ws), need, bufs) == 0, eng.L.sylph_last_error()
    torch.cuda.synchronize()
    assert outs[5][0].item() == 0 and outs[6][0].item() == 0  # no rows: count 0, status clear
