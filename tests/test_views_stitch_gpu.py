"""The stitching view merge on the GPU (sylph_stitch_views, Engine.stitch_views, the model's route to it) against the numpy reference
of tests/views_stitch_ref.py.  Every comparison is exact.  The hand-made pools live in one 4000 x 4000 source under two kinds of
views: A = the left half (its right border, x = 2000, lies inside the source) and B = the right 2400 columns (its left border,
x = 1600); both are full height, so only those two borders cut.  Boxes have integer coordinates; every pool passes
views_stitch_ref.assert_margins on the CPU (all same-class pairs and every rule-4b test at least 1e-3 from their thresholds: here
the ratios are 0, 1 or far from 0.5 and 0.6), and every test asserts on the reference's trace that the walks do what it claims."""
import ctypes

import numpy as np
import pytest
import torch

import views_large_ref as LR
import views_ref as VR
import views_stitch_ref as SR
from sylph_amd import views as V
from test_views_gpu import _assert_merged, _assert_model, _codes, _composition, _engine, _model, _rows
from test_views_large_gpu import _big_source, _old_kernel_pools
from test_views_stitch_cpu import scene

pytestmark = pytest.mark.gpu

THR = 0.6
CHUNK, KEPT_LDS = 64, 2048  # csrc/kernels.h: MERGE_LARGE_CHUNK, MERGE_LARGE_KEPT_LDS
HW = (4000, 4000)
CROP = {"A": (0, 0, 2000, 4000), "B": (1600, 0, 2400, 4000)}
F = np.float32


@pytest.fixture(scope="module")
def eng():
    e = _engine("bf16", None, **{"MODEL.FCOS.NMS_TH": THR, "MODEL.FCOS.POST_NMS_TOPK_TEST": 100})
    yield e
    e.close()


# ---- the pieces of a hand-made pool: (box in source pixels, kind of the view it comes from) -------------------------------------------
def filler(f):
    """a 10 x 10 box of its own in the interior of view A: cut by nothing, meets no other piece"""
    x, y = 10 + 20 * (f % 70), 10 + 20 * (f // 70)
    assert y < 1990
    return [x, y, x + 10, y + 10], "A"


def triple(t):
    """One object across the strip 1600 ... 2000, band t: K1 = its last 100 columns in A (cut at x = 2000), K2 = its first 100 columns
    in B (cut at x = 1600), J = the strip's whole width as A sees it (cut).  K1 and K2 do not meet; J matches both with ratio 1; the
    hull of K1 and J holds all of K2."""
    y = 2000 + 20 * t
    assert y + 10 < 3998
    return {"K1": ([1900, y, 2000, y + 10], "A"), "K2": ([1600, y, 1700, y + 10], "B"), "J": ([1600, y, 2000, y + 10], "A")}


def layout(rows, per_view, source=0, flip=()):
    """rows = [(box, kind, score, class)] -> (table, rows per view) for SR.build_pool: per kind, views of per_view rows in the order
    the rows come; the A views first.  flip: the kinds whose views are mirrored."""
    table, per = [], []
    for kind in "AB":
        mine = [(b, s, c) for b, k, s, c in rows if k == kind]
        for k0 in range(0, len(mine), per_view):
            table.append({"source": source, "crop": CROP[kind], "flip": kind in flip})
            per.append(mine[k0:k0 + per_view])
    return table, per


def ranked_pool(pieces, per_view=100, cls=3, flip=()):
    """pieces[pos] = (box, kind): one class, strictly descending scores, so pos IS the rule-3 position -> pool"""
    rows = [(b, k, 0.95 - 1e-4 * pos, cls) for pos, (b, k) in enumerate(pieces)]
    table, per = layout(rows, per_view, flip=flip)
    return SR.build_pool(table, per, per_view)


def checked(pool, n_src=1, sizes=(HW,), thr=THR, sthr=0.5, border=2.0):
    """the margins on the CPU -> the reference at K = 0"""
    return SR.assert_margins(pool, n_src, list(sizes), thr, sthr, border)


def run(eng, pool, n_src=1, sizes=(HW,), topk=0, thr=THR, sthr=0.5, border=2.0, max_out=None, what=""):
    table, boxes, scores, classes, counts = pool
    K = int(eng.sc.post_nms_topk) if topk is None else topk
    want = SR.stitch_ref(table, boxes, scores, classes, counts, n_src, list(sizes), thr, K, sthr, border)
    if max_out is None:
        max_out = max(len(w["scores"]) for w in want) + 3
    got = eng.stitch_views(table, _rows(boxes, scores, classes, counts), list(sizes), sthr, border, max_out=max_out, n_src=n_src, topk=topk)
    _assert_merged(got, want, what)
    for s, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g["stitched"].cpu(), torch.from_numpy(w["stitched"])), f"{what}: source {s}: stitched differs"
    return got, want


def _pos(ref):
    """pool index -> rule-3 position"""
    pos = np.empty(len(ref["order"]), dtype=np.int64)
    pos[ref["order"]] = np.arange(len(ref["order"]))
    return pos


# ------------------------------------------------------------------------------------------------ 1: no cut row = the large merge
def _uncut(pool, n_src, sizes, border):
    """the rows of a pool that rule 0 does not flag, closed up per view (a subset: the pool's IoU margin from NMS_TH still holds)"""
    table, boxes, scores, classes, counts = pool
    boxes, scores, classes, counts = boxes.copy(), scores.copy(), classes.copy(), counts.copy()
    removed = 0
    for v, t in enumerate(table):
        n = int(counts[v])
        sb = np.array([VR.to_source(boxes[v, r], t) for r in range(n)], dtype=F).reshape(-1, 4)
        keep = ~V.cut_flags(t, sizes[t["source"]], sb, border)
        k = int(keep.sum())
        boxes[v, :k], scores[v, :k], classes[v, :k] = boxes[v, :n][keep], scores[v, :n][keep], classes[v, :n][keep]
        counts[v] = k
        removed += n - k
    return (table, boxes, scores, classes, counts), removed


@pytest.fixture(scope="module")
def uncut_pools():
    """_old_kernel_pools() are drawn around objects, not clipped to their crops: rows leave their crops on the left and on the top,
    where most crops have an inner border (x0, y0 > 0), so rule 0 flags some of them whatever border_px is.  Those rows are taken out;
    the rest, under the same tables, is the pool without a cut row.  Sources are 300 x 300: every crop lies inside."""
    out = {}
    for name, (pool, n_src) in _old_kernel_pools().items():
        sizes = [(300, 300)] * n_src
        sub, removed = _uncut(pool, n_src, sizes, 2.0)
        assert 0 < removed < int(pool[4].sum()) // 2, name
        assert all(r["cut_rows"] == 0 for r in SR.stitch_ref(*sub, n_src, sizes, THR, 0)), name
        out[name] = (sub, n_src, sizes)
    return out


@pytest.mark.parametrize("thr", [0.6, 0.0])
@pytest.mark.parametrize("K", [100, 7, 0])
def test_without_cut_rows_it_equals_the_large_merge(uncut_pools, thr, K):
    e = _engine("bf16", None, **{"MODEL.FCOS.NMS_TH": thr, "MODEL.FCOS.POST_NMS_TOPK_TEST": K})
    for name, (pool, n_src, sizes) in uncut_pools.items():
        table, boxes, scores, classes, counts = pool
        want = LR.merge_large_ref(table, boxes, scores, classes, counts, n_src, thr, K)
        total = int(np.sum(counts))
        if thr > 0:
            assert sum(w["kept"] for w in want) < total, f"{name}: NMS has no work"
        if K == 7:
            assert max(w["kept"] for w in want) > K, f"{name}: rule 5 has no work at K = {K}"
        large = e.merge_views_large(table, _rows(boxes, scores, classes, counts), max_out=total, n_src=n_src)
        new = e.stitch_views(table, _rows(boxes, scores, classes, counts), sizes, max_out=total, n_src=n_src)
        for a, b in zip(large, new):
            for k in ("pred_boxes", "scores", "pred_classes", "view_index", "view_row"):
                assert torch.equal(a[k], b[k]), f"{name}, NMS_TH {thr}, K {K}: {k} differs from the large merge"
            assert bool((b["stitched"] == 1).all()) and b["stitched"].numel() == b["scores"].numel()
        _assert_merged(new, want, f"{name}, NMS_TH {thr}, K {K}")
    e.close()


# ------------------------------------------------------------------------------------------------ 2: segments around the chunk
def chunk_pieces(n):
    """n rows of one class by rule-3 position -> pieces, the triples' positions {name: (K1, K2, J)}, (dup position, its filler's)"""
    pieces = [filler(p) for p in range(n)]
    triples, dup = {}, None
    if n == 1:
        pieces[0] = triple(0)["K1"]
    if n >= 63:
        triples["inside chunk 0"] = (5, 20, 40)
        dup = (50, 3)
    if n == 65:
        triples["keepers in chunk 0, row in chunk 1"] = (7, 25, 64)
    if n >= 127:
        triples["keeper in chunk 0, a later one and the row in chunk 1"] = (10, 66, 70)
        triples["inside chunk 1"] = (80, 90, 100)
    if n == 129:
        triples["keepers in two groups of 64, row in chunk 2"] = (12, 120, 128)
    for t, (k1, k2, j) in enumerate(triples.values()):
        tr = triple(t)
        pieces[k1], pieces[k2], pieces[j] = tr["K1"], tr["K2"], tr["J"]
    if dup:
        pieces[dup[0]] = filler(dup[1])
    return pieces, triples, dup


@pytest.mark.parametrize("n", [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK + 1])
def test_segments_around_the_chunk_and_the_first_keeper(eng, n):
    pieces, triples, dup = chunk_pieces(n)
    pool = ranked_pool(pieces, per_view=50)
    ref = checked(pool)[0]
    order, pos = ref["order"], _pos(ref)
    trace = {row: (keeper, matches, cut_pair) for row, keeper, matches, cut_pair in ref["trace"]}
    rank = {row: r for r, row in enumerate(ref["kept_rows"])}
    for name, (k1, k2, j) in triples.items():
        keeper, matches, cut_pair = trace[order[j]]
        assert keeper == order[k1] and order[k2] in matches and cut_pair, f"{name}: the row has two kept matches and goes to the first"
        assert (order[k2], order[k1]) in ref["drops"], f"{name}: rule 4b drops the second fragment"
        if "chunk 1" in name and "inside" not in name:
            assert j // CHUNK == 1 and k1 // CHUNK == 0
        if "a later one" in name:
            assert k2 // CHUNK == 1 and k2 < j
        if "inside" in name:
            assert k1 // CHUNK == k2 // CHUNK == j // CHUNK
        if "two groups" in name:
            assert rank[order[k1]] // 64 == 0 and rank[order[k2]] // 64 == 1 and j // CHUNK == 2
    if dup:
        assert trace[order[dup[0]]] == (order[dup[1]], [order[dup[1]]], False), "an uncut pair: plain NMS suppresses"
    assert (ref["absorbed"], ref["dropped"], ref["suppressed"]) == (len(triples), len(triples), 1 if dup else 0)
    assert int(pool[4].sum()) == n and ref["cut_rows"] == (3 * len(triples) if n > 1 else 1)
    got, want = run(eng, pool, what=f"one class, {n} rows")
    assert sorted(got[0]["stitched"].tolist(), reverse=True)[:len(triples)] == [3] * len(triples)
    run(eng, pool, topk=7, what=f"one class, {n} rows, K 7")


# ------------------------------------------------------------------------------------------------ 3: kept boxes around the LDS list
def lds_pieces(n_kept):
    """n_kept rows that rule 4a keeps (positions = ranks), then the fragments J of the triples, then 40 copies of fillers.
    -> pieces, triples {name: (rank of K1, rank of K2 or None, position of J)}"""
    plan = {"in the list": (100, 200)}
    if n_kept == KEPT_LDS - 1:
        plan["the last kept box"] = (KEPT_LDS - 2, None)
    if n_kept == KEPT_LDS:
        plan["the last box of the list"] = (KEPT_LDS - 1, None)
    if n_kept == KEPT_LDS + 1:
        plan["the last box of the list, its second fragment the first spilled box"] = (KEPT_LDS - 1, KEPT_LDS)
    if n_kept == KEPT_LDS + 70:
        plan["the last box of the list"] = (KEPT_LDS - 1, None)
        plan["the first spilled box, its second fragment spilled too"] = (KEPT_LDS, KEPT_LDS + 52)
        plan["the last kept box, spilled"] = (n_kept - 1, None)
    pieces = [filler(p) for p in range(n_kept)]
    triples = {}
    for t, (name, (k1, k2)) in enumerate(plan.items()):
        tr = triple(t)
        pieces[k1] = tr["K1"]
        if k2 is not None:
            pieces[k2] = tr["K2"]
        triples[name] = (k1, k2, len(pieces))
        pieces.append(tr["J"])
    rng = np.random.RandomState(n_kept)
    taken = {k for k1, k2, _ in triples.values() for k in (k1, k2)}
    free = [p for p in range(n_kept) if p not in taken]
    for p in free[-20:] + [free[i] for i in rng.choice(len(free) - 20, 20, replace=False)]:
        pieces.append(filler(p))
    return pieces, triples


@pytest.mark.parametrize("n_kept", [KEPT_LDS - 1, KEPT_LDS, KEPT_LDS + 1, KEPT_LDS + 70])
def test_kept_boxes_around_the_lds_list(eng, n_kept):
    """Union boxes that grow in LDS and in the spill, a rule-4b drop against a survivor in the list and against a spilled one, copies
    suppressed by kept boxes beyond the list."""
    pieces, triples = lds_pieces(n_kept)
    pool = ranked_pool(pieces, per_view=100)
    ref = checked(pool)[0]
    order = ref["order"]
    assert ref["kept"] == n_kept and ref["kept_rows"] == order[:n_kept].tolist(), "rank = position for the first n_kept rows"
    trace = {row: (keeper, cut_pair) for row, keeper, _, cut_pair in ref["trace"]}
    for name, (k1, k2, j) in triples.items():
        assert trace[order[j]] == (order[k1], True), name
        if k2 is not None:
            assert (order[k2], order[k1]) in ref["drops"], name
    n_drops = sum(k2 is not None for _, k2, _ in triples.values())
    assert (ref["absorbed"], ref["dropped"], ref["suppressed"]) == (len(triples), n_drops, 40)
    if n_kept == KEPT_LDS + 70:
        assert any(k1 >= KEPT_LDS and k2 is not None for k1, k2, _ in triples.values()), "a drop against a spilled survivor"
        assert sum(1 for row, keeper, _, cut_pair in ref["trace"] if not cut_pair and keeper in order[KEPT_LDS:n_kept]) >= 10
    got, _ = run(eng, pool, what=f"{n_kept} kept boxes")
    assert got[0]["scores"].numel() == n_kept - n_drops


# ------------------------------------------------------------------------------------------------ 4: pool sizes, sources, classes, ties
CLASS_IDS = np.array([0, 7, 65536, 2 ** 31 - 1, -5], dtype=np.int32)


def mixed_rows(n, seed):
    """n rows: 60 triples, 100 copies of fillers, fillers; a class per object out of CLASS_IDS; scores on 30 levels, so that scores tie
    across views and the order inside a triple is any"""
    rng = np.random.RandomState(seed)
    n_tri = min(60, n // 8)
    n_dup = min(100, n // 8)
    n_fill = n - 3 * n_tri - n_dup
    level = lambda: 0.05 + 0.9 * rng.randint(31) / 30.0
    rows = []
    fill_cls = CLASS_IDS[rng.randint(len(CLASS_IDS), size=n_fill)]
    for f in range(n_fill):
        rows.append(filler(f) + (level(), int(fill_cls[f])))
    for f in rng.choice(n_fill, n_dup, replace=False):
        rows.append(filler(f) + (level(), int(fill_cls[f])))
    for t in range(n_tri):
        c = int(CLASS_IDS[rng.randint(len(CLASS_IDS))])
        rows += [piece + (level(), c) for piece in triple(t).values()]
    return [rows[i] for i in rng.permutation(n)]


@pytest.mark.parametrize("n", [2047, 2048, 2049, 4097])
def test_pool_sizes_around_the_sorted_lengths(eng, n):
    """n views of one row: the pool is exactly n rows"""
    table, per = layout(mixed_rows(n, n), 1)
    pool = SR.build_pool(table, per, 1)
    assert len(table) == n and int(pool[4].sum()) == n
    ref = checked(pool)[0]
    assert ref["absorbed"] > 20 and ref["dropped"] > 5 and ref["suppressed"] > 20
    assert len(set(pool[2][:, 0].tolist())) <= 31, "scores tie across views"
    got, _ = run(eng, pool, topk=100, what=f"{n} rows")
    assert set(got[0]["pred_classes"].tolist()) <= set(CLASS_IDS.tolist()) and int(got[0]["pred_classes"].min()) == -5
    run(eng, pool, topk=0, what=f"{n} rows, K 0")


def test_three_sources_and_an_empty_one(eng):
    """sources 0 and 2 hold pools of their own under interleaved views, source 1 one view without rows"""
    t0, p0 = layout(mixed_rows(600, 1), 7, source=0)
    t2, p2 = layout(mixed_rows(500, 2), 7, source=2)
    table, per = [], []
    for k in range(max(len(t0), len(t2))):
        for t, p in ((t0, p0), (t2, p2)):
            if k < len(t):
                table.append(t[k])
                per.append(p[k])
        if k == 3:
            table.append({"source": 1, "crop": CROP["A"], "flip": False})
            per.append([])
    pool = SR.build_pool(table, per, 7)
    sizes = [HW, HW, HW]
    ref = checked(pool, 3, sizes)
    assert [r["survivors"] > 0 for r in ref] == [True, False, True]
    assert all(r["absorbed"] > 0 and r["suppressed"] > 0 and r["dropped"] > 0 for r in (ref[0], ref[2]))
    got, _ = run(eng, pool, 3, sizes, topk=100, what="three sources")
    assert got[1]["scores"].numel() == 0
    again, _ = run(eng, pool, 3, sizes, topk=100, what="three sources, again")
    for a, b in zip(got, again):
        assert all(torch.equal(a[k], b[k]) for k in a), "the same call gives the same bits"


# ------------------------------------------------------------------------------------------------ 5: rule 5, truncation, counts
def topk_pieces():
    """a cut box at rank 3, 120 kept boxes in all, its fragment at the very end: in the second chunk, far below the seventh kept score"""
    pieces = [filler(p) for p in range(120)]
    tr = triple(0)
    pieces[3] = tr["K1"]
    pieces.append(tr["J"])
    return pieces


def test_a_late_fragment_grows_one_of_the_first_seven(eng):
    pool = ranked_pool(topk_pieces(), per_view=50)
    ref = checked(pool)[0]
    order = ref["order"]
    assert ref["trace"] == [(order[120], order[3], [order[3]], True)] and ref["kept"] == 120
    want = SR.stitch_ref(*pool, 1, [HW], THR, 7)[0]
    assert len(want["scores"]) == 7 and want["stitched"].tolist() == [1, 1, 1, 2, 1, 1, 1]
    assert want["pred_boxes"][3].tolist() == [1600.0, 2000.0, 2000.0, 2010.0], "the emitted box holds a row from behind the K-th kept score"
    assert pool[2][pool[2] > 0].min() < want["scores"][6] and 120 // CHUNK == 1
    got, _ = run(eng, pool, topk=7, what="K 7")
    assert got[0]["stitched"].tolist() == [1, 1, 1, 2, 1, 1, 1]
    run(eng, pool, topk=None, what="K None is POST_NMS_TOPK_TEST")
    # truncation: Engine.stitch_views raises on status bit 2 as the other merges do
    table, boxes, scores, classes, counts = pool
    with pytest.raises(RuntimeError, match="max_out"):
        eng.stitch_views(table, _rows(boxes, scores, classes, counts), [HW], max_out=119, topk=0)
    run(eng, pool, topk=0, max_out=120, what="max_out exactly the survivors, after a truncated call")


def _c_call(eng, pool, n_src, sizes, topk, max_out, sthr=0.5, border=2.0, ws=None, ws_bytes=None, crop_h=None, outs=None):
    """sylph_stitch_views itself -> rc, (boxes, scores, classes | view | row | stitched, counts | status)"""
    from sylph_amd.engine import _iarr, _ptr
    table, boxes, scores, classes, counts = pool
    nv, max_in = len(table), scores.shape[1]
    r = _rows(boxes, scores, classes, counts)
    fa = lambda vals: (ctypes.c_float * len(vals))(*[float(x) for x in vals])
    if outs is None:
        outs = (torch.zeros(n_src, max_out, 4, device="cuda"), torch.zeros(n_src, max_out, device="cuda"),
                torch.zeros(4, n_src, max_out, device="cuda", dtype=torch.int32), torch.full((n_src + 1,), -1, device="cuda", dtype=torch.int32))
    ob, osc, oi, tail = outs
    if ws is None:
        need = eng.L.sylph_stitch_views_bytes(n_src, nv, max_in)
        ws = torch.empty(need, device="cuda", dtype=torch.uint8)
        ws_bytes = need if ws_bytes is None else ws_bytes
    rc = eng.L.sylph_stitch_views(eng._ctx, n_src, nv, _iarr([t["source"] for t in table]), fa([t["crop"][0] for t in table]),
                                  fa([t["crop"][1] for t in table]), fa([t["crop"][2] for t in table]),
                                  fa([t["crop"][3] for t in table] if crop_h is None else crop_h), _iarr([1 if t["flip"] else 0 for t in table]),
                                  fa([s[1] for s in sizes]), fa([s[0] for s in sizes]), max_in, _ptr(r["boxes"]), _ptr(r["scores"]),
                                  _ptr(r["classes"]), _ptr(r["counts"]), sthr, border, topk, max_out, _ptr(ob), _ptr(osc), _ptr(oi[0]), _ptr(oi[1]),
                                  _ptr(oi[2]), _ptr(oi[3]), _ptr(tail), ctypes.c_void_p(tail.data_ptr() + 4 * n_src),
                                  _ptr(ws) if isinstance(ws, torch.Tensor) else ws, ws_bytes)
    return rc, outs


def test_a_truncated_source_holds_its_first_rows(eng):
    """the C entry: status bit 1 and the first max_out rows in order, the grown box among them"""
    pool = ranked_pool(topk_pieces(), per_view=50)
    want = SR.stitch_ref(*pool, 1, [HW], THR, 0, max_out=64)[0]
    assert want["truncated"] and want["stitched"][3] == 2
    rc, (ob, osc, oi, tail) = _c_call(eng, pool, 1, [HW], 0, 64)
    assert rc == 0, eng.L.sylph_last_error()
    assert tail.tolist() == [64, 2]
    assert torch.equal(ob[0].cpu(), torch.from_numpy(want["pred_boxes"])) and torch.equal(osc[0].cpu(), torch.from_numpy(want["scores"]))
    assert torch.equal(oi[1, 0].cpu().long(), torch.from_numpy(want["view_index"]))
    assert torch.equal(oi[2, 0].cpu().long(), torch.from_numpy(want["view_row"]))
    assert torch.equal(oi[3, 0].cpu().long(), torch.from_numpy(want["stitched"]))


def test_counts_outside_the_rows_are_clamped(eng):
    table, per = layout(mixed_rows(600, 5), 20)
    pool = SR.build_pool(table, per, 20)
    table, boxes, scores, classes, counts = pool
    assert len(table) > 6 and (counts[:6] == 20).all()
    wild, clamped = counts.copy(), counts.copy()
    wild[0], wild[3], wild[5] = 20 + 1, -1, 2 ** 31 - 1
    clamped[3] = 0
    small = (table, boxes, scores, classes, clamped)
    ref = checked(small)[0]
    assert ref["absorbed"] > 0 and ref["suppressed"] > 0
    want = SR.stitch_ref(*small, 1, [HW], THR, 100)
    got = eng.stitch_views(table, _rows(boxes, scores, classes, wild), [HW], max_out=700, topk=100)
    _assert_merged(got, want, "clamped counts")
    assert torch.equal(got[0]["stitched"].cpu(), torch.from_numpy(want[0]["stitched"]))


# ------------------------------------------------------------------------------------------------ 6: mirrored views
def test_flipped_tiles_are_cut_on_the_mirrored_side(eng):
    """The B views mirrored: their inner border is the crop's LEFT side in the source, the RIGHT side of the rows they return (x = the
    crop's width in crop pixels).  The result is that of the unmirrored pool; then both kinds mirrored."""
    pieces, triples, _ = chunk_pieces(129)
    plain = ranked_pool(pieces, per_view=50)
    want = checked(plain)[0]
    for flip in (("B",), ("A", "B")):
        pool = ranked_pool(pieces, per_view=50, flip=flip)
        table, boxes, _, _, counts = pool
        b_views = [v for v, t in enumerate(table) if t["crop"] == CROP["B"]]
        assert all(table[v]["flip"] for v in b_views)
        assert all((boxes[v, :counts[v], 2] == 2400).all() and (boxes[v, :counts[v], 0] > 2).all() for v in b_views), "cut on the mirrored side"
        ref = checked(pool)[0]
        assert ref["cut_rows"] == 3 * len(triples) and ref["absorbed"] == len(triples) == ref["dropped"]
        for k in ("pred_boxes", "scores", "view_index", "view_row", "stitched"):
            assert np.array_equal(ref[k], want[k]), k
        run(eng, pool, what=f"mirrored {flip}")


# ------------------------------------------------------------------------------------------------ 7: a tiled scene
@pytest.mark.parametrize("name", ["40-420 px", "300-1300 px"])
def test_a_tiled_scene_comes_back_whole(eng, name):
    """tests/test_views_stitch_cpu.py's scene on the device: one box per object, equal to its ground truth, `stitched` equal too"""
    pool, gt, hw = scene(name, 0)
    ref = checked(pool, sizes=[hw])[0]
    assert ref["absorbed"] > 0 and ref["suppressed"] > 0 and (ref["dropped"] > 0 or name == "40-420 px")
    got, _ = run(eng, pool, sizes=[hw], topk=0, what=name)
    assert {tuple(b) for b in got[0]["pred_boxes"].tolist()} == {tuple(g) for g in gt.tolist()} and got[0]["scores"].numel() == len(gt)
    large = eng.merge_views_large(pool[0], _rows(*pool[1:]), max_out=400, topk=0)
    assert large[0]["scores"].numel() > len(gt), "the plain merge keeps the pieces"


# ------------------------------------------------------------------------------------------------ 8: the model, end to end
@pytest.fixture(scope="module")
def sd():
    from sylph_amd import synthetic as W
    return W.synthetic_state_dict(0, depth=50)


def _stitched_composition(model, srcs, views, codes, sthr, border, monkeypatch):
    """_composition up to its numpy merge, whose rows then go through Engine.stitch_views -> merged (view_index in the input's own
    list), the reference's walk statistics on those rows"""
    seen = {}
    real = VR.merge_ref

    def spy(table, boxes, scores, classes, counts, n_src, thr, k):
        seen["pool"] = (table, boxes.copy(), scores.copy(), classes.copy(), counts.copy())
        return real(table, boxes, scores, classes, counts, n_src, thr, k)

    monkeypatch.setattr(VR, "merge_ref", spy)
    _composition(model, srcs, views, codes)
    monkeypatch.undo()
    table, boxes, scores, classes, counts = seen["pool"]
    sizes = [s.shape[:2] for s in srcs]
    ref = SR.stitch_ref(table, boxes, scores, classes, counts, len(srcs), sizes, float(model.cfg.MODEL.FCOS.NMS_TH), 0, sthr, border)
    merged = model.engine.stitch_views(table, _rows(boxes, scores, classes, counts), sizes, sthr, border, n_src=len(srcs))
    own = np.array([v["view"] for v in table])
    want = [{k: (own[d[k].cpu().numpy()] if k == "view_index" else d[k].cpu().numpy()) for k in d} for d in merged]
    return want, ref


def test_model_stitch_equals_the_composition(sd, monkeypatch):
    """A tiled input with "stitch" = the Engine steps of the composition plus Engine.stitch_views.  At the defaults (stitch_thr 0.5,
    border_px 2.0) the 31 views of the 330 x 440 source (seed 51) return rows that their crops' inner borders cut: decode clips to
    the crop, and a clipped box ends ON the border."""
    from sylph_amd.predictor import SylphPredictor
    model = _model("bf16", sd)
    src, views = _big_source()
    d0 = _codes(5, 42)
    kw = dict(class_code=d0, run_type="meta_learn_test_instance")
    batch = [{"image_u8": torch.from_numpy(src), "resize_hw": (96, 128), "views": views}]
    plain = model(batch, **kw)
    assert not plain[0]["instances"].has("stitched"), "without \"stitch\" the outputs are what they were"
    for stitch, (sthr, border) in ((True, (0.5, 2.0)), ({"thr": 0.3, "border": 4.0}, (0.3, 4.0))):
        got = model([dict(batch[0], stitch=stitch)], **kw)
        want, ref = _stitched_composition(model, [src], [views], d0, sthr, border, monkeypatch)
        assert ref[0]["cut_rows"] > 0, "the composition holds no cut row"
        assert ref[0]["absorbed"] + ref[0]["dropped"] > 0, f"stitching has no work on {ref[0]['cut_rows']} cut rows"
        _assert_model(got, want, [src])
        assert torch.equal(got[0]["instances"].stitched.cpu(), torch.from_numpy(want[0]["stitched"]))
        assert int(got[0]["instances"].stitched.max()) > 1
    # the predictor's arguments reach the merge (its constructor needs a checkpoint and class codes on disk: only _preprocess runs here)
    pred = SylphPredictor.__new__(SylphPredictor)
    pred.min_size, pred.max_size, pred.fused_preprocess, pred.input_format, pred._pinned = 64, 160, True, "BGR", {}
    pred.tiles, pred.tile_overlap, pred.max_detections, pred.stitch = (96, 96), 0.25, None, {"thr": 0.3, "border": 4.0}
    inputs = pred._preprocess(src)
    assert inputs["stitch"] == {"thr": 0.3, "border": 4.0} and inputs["views"] == views
    again = model([inputs], **kw)
    _assert_model(again, want, [src])
    assert torch.equal(again[0]["instances"].stitched.cpu(), torch.from_numpy(want[0]["stitched"]))
    pred.stitch = None
    assert "stitch" not in pred._preprocess(src)


def test_model_stitch_on_tta_views_is_the_plain_merge(sd):
    """full-frame views only: no row is cut"""
    from sylph_amd.views import tta_views
    from test_views_gpu import _u8
    model = _model("bf16", sd)
    src = _u8(96, 128, 31)
    views = tta_views(96, 128, (64, 96), 160, True)
    d0 = _codes(5, 42)
    kw = dict(class_code=d0, run_type="meta_learn_test_instance")
    batch = [{"image_u8": torch.from_numpy(src), "resize_hw": (96, 128), "views": views}]
    plain = model(batch, **kw)[0]["instances"]
    got = model([dict(batch[0], stitch=True)], **kw)[0]["instances"]
    assert len(got) == len(plain) > 0 and torch.equal(got.pred_boxes.tensor, plain.pred_boxes.tensor) and torch.equal(got.scores, plain.scores)
    assert torch.equal(got.view_index, plain.view_index) and torch.equal(got.view_row, plain.view_row) and bool((got.stitched == 1).all())


# ------------------------------------------------------------------------------------------------ 9: refusals by name
def test_refusals_by_name(eng, sd):
    pool = ranked_pool(topk_pieces(), per_view=50)
    nv = len(pool[0])
    outs = (torch.full((1, 8, 4), -7.0, device="cuda"), torch.full((1, 8), -7.0, device="cuda"),
            torch.full((4, 1, 8), -7, device="cuda", dtype=torch.int32), torch.full((2,), -7, device="cuda", dtype=torch.int32))
    err = lambda: eng.L.sylph_last_error()
    call = lambda **k: _c_call(eng, pool, 1, k.pop("sizes", [HW]), -1, 8, outs=outs, **k)[0]
    for sthr in (0.0, -0.5, 1.5, float("nan")):
        assert call(sthr=sthr) != 0 and b"stitch_thr" in err()
    for border in (-1.0, float("nan")):
        assert call(border=border) != 0 and b"border_px" in err()
    assert call(sizes=[(0, 4000)]) != 0 and b"sizes must be positive" in err() and b"source 0" in err()
    assert call(crop_h=[4000.0] * (nv - 1) + [0.0]) != 0 and b"sizes must be positive" in err() and b"crop of view" in err()
    assert call(sizes=[(4000, 1999)]) != 0 and b"leaves its" in err()
    assert call(crop_h=[4001.0] + [4000.0] * (nv - 1)) != 0 and b"leaves its" in err()
    need = eng.L.sylph_stitch_views_bytes(1, nv, 50)
    ws = torch.empty(need, device="cuda", dtype=torch.uint8)
    assert call(ws=0, ws_bytes=need) != 0 and b"workspace is NULL" in err()
    assert call(ws=ws, ws_bytes=need - 1) != 0 and b"sylph_stitch_views_bytes asks for" in err()
    big = (pool[0] * 2000,) + tuple(np.zeros((1,) + a.shape[1:], a.dtype) for a in pool[1:4]) + (np.zeros(1, np.int32),)
    from sylph_amd.engine import _iarr, _ptr
    n_big = len(big[0])
    assert n_big * 200 > 1048576
    fa, f0, one = (ctypes.c_float * n_big)(*([1.0] * n_big)), (ctypes.c_float * n_big)(*([0.0] * n_big)), (ctypes.c_float * 1)(1.0)
    z = torch.zeros(16, device="cuda")
    rc = eng.L.sylph_stitch_views(eng._ctx, 1, n_big, _iarr([0] * n_big), f0, f0, fa, fa, _iarr([0] * n_big), one, one, 200, _ptr(z), _ptr(z), _ptr(z),
                                  _ptr(z), 0.5, 2.0, -1, 8, _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2][0]), _ptr(outs[2][1]), _ptr(outs[2][2]),
                                  _ptr(outs[2][3]), _ptr(outs[3]), ctypes.c_void_p(outs[3].data_ptr() + 4), _ptr(ws), need)
    assert rc != 0 and b"MERGE_LARGE_POOL_CAP" in err()
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in outs), "a refused call writes nothing"
    assert call(ws=ws, ws_bytes=need) == 0, err()
    torch.cuda.synchronize()
    assert outs[3].tolist() == [8, 2]  # more than 8 survivors: truncated, and said so
    # Engine and model
    table, boxes, scores, classes, counts = pool
    with pytest.raises(RuntimeError, match="stitch_thr"):
        eng.stitch_views(table, _rows(boxes, scores, classes, counts), [HW], stitch_thr=0.0)
    with pytest.raises(ValueError, match="source sizes"):
        eng.stitch_views(table, _rows(boxes, scores, classes, counts), [HW, HW])
    model = _model("bf16", sd)
    src, views = _big_source()
    kw = dict(class_code=_codes(5, 42), run_type="meta_learn_test_instance")
    one = {"image_u8": torch.from_numpy(src), "resize_hw": (96, 128)}
    with pytest.raises(ValueError, match="\"stitch\" joins"):  # no views, no merge: refused, not ignored
        model([dict(one, stitch=True)], **kw)
    with pytest.raises(ValueError, match="disagree on \"stitch\""):
        model([dict(one, views=views, stitch=True), dict(one, views=views, stitch={"thr": 0.4})], **kw)
    with pytest.raises(ValueError, match="disagree on \"stitch\""):
        model([dict(one, views=views, stitch=True), dict(one, views=views)], **kw)
    with pytest.raises(ValueError, match="thr"):
        model([dict(one, views=views, stitch={"thr": 2.0})], **kw)
