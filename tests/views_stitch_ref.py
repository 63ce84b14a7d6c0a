"""Reference of the stitching view merge (tests/test_views_stitch_cpu.py, tests/test_views_stitch_gpu.py), CPU only: the rules 0 - 5
above sylph_stitch_views (include/sylph_hip.h) as greedy walks in float32 numpy, in the style of tests/views_large_ref.py.  Rule 0 is
sylph_amd.views.cut_flags, the one host helper the package and this reference share; nothing else comes from the library.
Also here: the pool builder of the hand-made pools (source boxes -> per-view rows) and the margin check every pool has to pass on the
CPU before a device result is compared with the reference: no same-class pair of a source within 1e-3 of the threshold that applies
to it, and no rule-4b test that the walk makes within 1e-3 of stitch_thr."""
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from sylph_amd.views import cut_flags

F = np.float32
MARGIN = 1e-3


def source_rows(view_table, boxes, scores, classes, counts, s):
    """rules 1 and 2 for source s -> view index, row index, source boxes, scores, classes of its pool"""
    max_in = scores.shape[1]
    vs = [v for v in range(len(view_table)) if view_table[v]["source"] == s]
    n_rows = [min(max(int(counts[v]), 0), max_in) for v in vs]
    vi = np.repeat(np.asarray(vs, dtype=np.int64), n_rows)
    ri = np.concatenate([np.arange(n, dtype=np.int64) for n in n_rows]) if vs else np.zeros(0, dtype=np.int64)
    b = boxes[vi, ri].astype(F).reshape(-1, 4)
    flip = np.array([bool(view_table[v].get("flip", False)) for v in vi], dtype=bool)
    cw = np.array([view_table[v]["crop"][2] for v in vi], dtype=F)
    x0 = np.array([view_table[v]["crop"][0] for v in vi], dtype=F)
    y0 = np.array([view_table[v]["crop"][1] for v in vi], dtype=F)
    x1 = np.where(flip, (cw - b[:, 2]).astype(F), b[:, 0])
    x2 = np.where(flip, (cw - b[:, 0]).astype(F), b[:, 2])
    sb = np.stack([(x1 + x0).astype(F), (b[:, 1] + y0).astype(F), (x2 + x0).astype(F), (b[:, 3] + y0).astype(F)], axis=1).reshape(-1, 4)
    return vi, ri, sb, scores[vi, ri].astype(F), classes[vi, ri].astype(np.int64)


def _areas(b):
    return ((b[..., 2] - b[..., 0]).astype(F) * (b[..., 3] - b[..., 1]).astype(F)).astype(F)


def _inter(many, one):
    w = np.maximum(F(0), (np.minimum(many[:, 2], one[2]) - np.maximum(many[:, 0], one[0])).astype(F))
    h = np.maximum(F(0), (np.minimum(many[:, 3], one[3]) - np.maximum(many[:, 1], one[1])).astype(F))
    return (w * h).astype(F)


class _Grow:
    """the kept rows of one class: boxes, areas, cut flags, pool indices"""

    def __init__(self):
        self.box, self.area, self.cut, self.idx, self.n = np.empty((16, 4), F), np.empty(16, F), np.zeros(16, bool), np.empty(16, np.int64), 0

    def add(self, box, area, cut, idx):
        if self.n == len(self.area):
            self.box, self.area = np.concatenate([self.box, np.empty_like(self.box)]), np.concatenate([self.area, np.empty_like(self.area)])
            self.cut, self.idx = np.concatenate([self.cut, np.zeros_like(self.cut)]), np.concatenate([self.idx, np.empty_like(self.idx)])
        self.box[self.n], self.area[self.n], self.cut[self.n], self.idx[self.n] = box, area, cut, idx
        self.n += 1


def stitch_ref(view_table: List[Dict], boxes: np.ndarray, scores: np.ndarray, classes: np.ndarray, counts: np.ndarray, n_src: int,
               source_sizes: Sequence[Tuple[int, int]], thr: float, K: int, stitch_thr: float = 0.5, border_px: float = 2.0,
               max_out: Optional[int] = None, no_cut: bool = False) -> List[Dict]:
    """Inputs as views_large_ref.merge_large_ref plus source_sizes[s] = (height, width) -> per source its keys plus "stitched", and
    what the walks did: "cut_rows" (rule 0), "kept" (rows rule 4a kept), "absorbed" (cut pairs that grew a union box), "suppressed"
    (uncut pairs), "dropped" (rule 4b), "margin" (the smallest distance of a test the walks made from its threshold), and in indices
    of the source's pool: "order" (rule 3), "kept_rows" (in keep order), "trace" (per absorbed or suppressed row: the row, its keeper,
    every kept row that matched it, whether the pair was a cut pair), "drops" (per dropped row: the row, the survivor that holds it).
    no_cut: every cut flag false, whatever rule 0 says."""
    thr32, sthr = F(thr), F(stitch_thr)
    out = []
    for s in range(n_src):
        vi, ri, sb, sc, cl = source_rows(view_table, boxes, scores, classes, counts, s)
        n = len(sc)
        # rule 0
        cut = np.zeros(n, dtype=bool)
        if not no_cut:
            for v in np.unique(vi):
                m = vi == v
                cut[m] = cut_flags(view_table[int(v)], source_sizes[s], sb[m], border_px)
        order = np.argsort(-sc, kind="stable")  # rule 3
        area = _areas(sb)
        U = sb.copy()
        count = np.zeros(n, dtype=np.int64)
        per_class: Dict[int, _Grow] = {}
        kept = []
        absorbed = suppressed = dropped = 0
        trace, drops = [], []  # (row, its keeper, every kept row that matched it, cut pair?) / (dropped row, the survivor that holds it), pool indices
        margin = np.inf
        # rule 4a
        for i in order:
            slot = per_class.get(cl[i])
            if slot is None:
                slot = per_class[cl[i]] = _Grow()
            m = slot.n
            if m:
                inter = _inter(slot.box[:m], sb[i])
                pair_cut = slot.cut[:m] | cut[i]
                with np.errstate(divide="ignore", invalid="ignore"):
                    ios = (inter / np.minimum(slot.area[:m], area[i])).astype(F)
                    iou = (inter / ((slot.area[:m] + area[i]).astype(F) - inter).astype(F)).astype(F)
                hit = np.where(pair_cut, ios > sthr, (iou > thr32) if thr > 0 else False)
                dist = np.where(pair_cut, np.abs(ios - sthr), np.abs(iou - thr32) if thr > 0 else np.inf)
                if np.isfinite(dist).any():
                    margin = min(margin, float(np.nanmin(dist)))
                if bool(hit.any()):
                    k = int(np.argmax(hit))  # the first kept row, in keep order, that matches
                    keeper = slot.idx[k]
                    trace.append((int(i), int(keeper), slot.idx[:m][hit].tolist(), bool(pair_cut[k])))
                    if pair_cut[k]:
                        U[keeper] = [min(U[keeper][0], sb[i][0]), min(U[keeper][1], sb[i][1]), max(U[keeper][2], sb[i][2]), max(U[keeper][3], sb[i][3])]
                        count[keeper] += 1
                        absorbed += 1
                    else:
                        suppressed += 1
                    continue
            slot.add(sb[i], area[i], cut[i], i)
            kept.append(i)
        n_kept = len(kept)
        # rule 4b: drop only
        surv_of: Dict[int, List[int]] = {}
        survivors = []
        for k in kept:
            mine = surv_of.setdefault(cl[k], [])
            if cut[k] and mine:
                with np.errstate(divide="ignore", invalid="ignore"):
                    share = (_inter(U[mine], sb[k]) / area[k]).astype(F)
                if np.isfinite(share).any():
                    margin = min(margin, float(np.nanmin(np.abs(share - sthr))))
                hit = share > sthr
                if bool(hit.any()):
                    count[mine[int(np.argmax(hit))]] += 1
                    drops.append((int(k), int(mine[int(np.argmax(hit))])))
                    dropped += 1
                    continue
            mine.append(k)
            survivors.append(k)
        survivors = np.asarray(survivors, dtype=np.int64)
        n_surv = len(survivors)
        # rule 5
        if K > 0 and n_surv > K:
            kth = sc[survivors[K - 1]]
            survivors = np.concatenate([survivors[:K], survivors[K:][sc[survivors[K:]] == kth]])
        truncated = max_out is not None and len(survivors) > max_out
        if truncated:
            survivors = survivors[:max_out]
        out.append({"pred_boxes": U[survivors].reshape(-1, 4), "scores": sc[survivors], "pred_classes": cl[survivors], "view_index": vi[survivors],
                    "view_row": ri[survivors], "stitched": 1 + count[survivors], "truncated": truncated, "kept": n_kept, "survivors": n_surv,
                    "cut_rows": int(cut.sum()), "absorbed": absorbed, "suppressed": suppressed, "dropped": dropped, "margin": margin,
                    "order": order, "kept_rows": kept, "trace": trace, "drops": drops})
    return out


def pair_margin(view_table, boxes, scores, classes, counts, n_src, source_sizes, thr, stitch_thr, border_px) -> float:
    """The smallest distance of a same-class pair of a source from the threshold that applies to it: intersection over the smaller box
    from stitch_thr for a pair with a cut row, IoU from NMS_TH (thr > 0) for any other.  Float32, the reference's arithmetic, ALL
    pairs -- also those no walk compares."""
    best = np.inf
    for s in range(n_src):
        vi, ri, sb, sc, cl = source_rows(view_table, boxes, scores, classes, counts, s)
        cut = np.zeros(len(sc), dtype=bool)
        for v in np.unique(vi):
            m = vi == v
            cut[m] = cut_flags(view_table[int(v)], source_sizes[s], sb[m], border_px)
        area = _areas(sb)
        for c in np.unique(cl):
            idx = np.nonzero(cl == c)[0]
            for k0 in range(0, len(idx), 256):
                a = idx[k0:k0 + 256]
                w = np.maximum(F(0), np.minimum(sb[a, None, 2], sb[None, idx, 2]) - np.maximum(sb[a, None, 0], sb[None, idx, 0]))
                h = np.maximum(F(0), np.minimum(sb[a, None, 3], sb[None, idx, 3]) - np.maximum(sb[a, None, 1], sb[None, idx, 1]))
                inter = (w * h).astype(F)
                with np.errstate(divide="ignore", invalid="ignore"):
                    ios = inter / np.minimum(area[a, None], area[None, idx])
                    iou = inter / ((area[a, None] + area[None, idx]).astype(F) - inter)
                pair_cut = cut[a, None] | cut[None, idx]
                dist = np.where(pair_cut, np.abs(ios - F(stitch_thr)), np.abs(iou - F(thr)) if thr > 0 else np.inf)
                dist[a[:, None] == idx[None, :]] = np.inf
                if np.isfinite(dist).any():
                    best = min(best, float(np.nanmin(dist)))
    return best


def assert_margins(pool, n_src, source_sizes, thr, stitch_thr=0.5, border_px=2.0):
    """the condition on a pool: every same-class pair and every rule-4b test at least MARGIN from its threshold -> the reference's result at K = 0"""
    table, boxes, scores, classes, counts = pool
    got = pair_margin(table, boxes, scores, classes, counts, n_src, source_sizes, thr, stitch_thr, border_px)
    assert got >= MARGIN, f"a same-class pair is {got:.2e} from its threshold"
    ref = stitch_ref(table, boxes, scores, classes, counts, n_src, source_sizes, thr, 0, stitch_thr, border_px)
    walk = min(r["margin"] for r in ref)
    assert walk >= MARGIN, f"a test of the walks is {walk:.2e} from its threshold"
    return ref


def build_pool(view_table: List[Dict], rows: Sequence[Sequence], max_in: int):
    """rows[v] = [(source box, score, class), ...] of view v, boxes in SOURCE pixels -> (table, boxes, scores, classes, counts) with the
    boxes in the view's own (possibly mirrored) crop pixels, the rows of a view in descending score order as decode leaves them.
    The way back (rule 1) must give the source box again, bit for bit: integer and half-integer coordinates do."""
    V = len(view_table)
    boxes, scores = np.zeros((V, max_in, 4), F), np.zeros((V, max_in), F)
    classes, counts = np.zeros((V, max_in), np.int32), np.zeros(V, np.int32)
    for v, (t, rs) in enumerate(zip(view_table, rows)):
        assert len(rs) <= max_in
        rs = sorted(rs, key=lambda r: -float(r[1]))  # (stable)
        x0, y0, cw = (F(q) for q in t["crop"][:3])
        for r, (sb, sc, c) in enumerate(rs):
            sb = np.asarray(sb, dtype=F)
            b = np.array([sb[0] - x0, sb[1] - y0, sb[2] - x0, sb[3] - y0], dtype=F)
            if t.get("flip", False):
                b = np.array([cw - b[2], b[1], cw - b[0], b[3]], dtype=F)
            boxes[v, r], scores[v, r], classes[v, r] = b, F(sc), c
        counts[v] = len(rs)
    for s in range(max(t["source"] for t in view_table) + 1):
        vi, ri, sb, _, _ = source_rows(view_table, boxes, scores, classes, counts, s)
        want = {v: sorted(rows[v], key=lambda r: -float(r[1])) for v in set(vi.tolist())}
        for v, r, b in zip(vi, ri, sb):
            assert np.array_equal(b, np.asarray(want[int(v)][int(r)][0], dtype=F)), "the source box does not survive the way to the crop and back"
    return view_table, boxes, scores, classes, counts


def tiled_scene(seed: int, lo: int, hi: int, n_obj: int, full_score: Tuple[float, float], H: int = 3000, W: int = 4000, tile: int = 800,
                overlap: float = 0.2, visible: float = 0.2, flipped: Sequence[int] = ()):
    """An H x W source under tile-pixel tiles with the full frame first (sylph_amd.views.tile_views); n_obj disjoint ground-truth boxes
    of lo ... hi - 1 pixels a side at integer positions; every view returns ground truth INTERSECTED with its crop for the objects it
    sees at least `visible` of, one class.  A tile's score grows with the visible share; the full frame scores full_score[0] +
    full_score[1] * u.  The views listed in `flipped` are mirrored, their rows with them.
    -> (pool, ground truth (n, 4) float32, (H, W))"""
    from sylph_amd.views import tile_views
    rng = np.random.default_rng(seed)
    views = tile_views(H, W, (tile, tile), overlap, None, 1333, full_frame=True)
    gts: List[np.ndarray] = []
    tries = 0
    while len(gts) < n_obj and tries < 20000:
        tries += 1
        w, h = int(rng.integers(lo, hi)), int(rng.integers(lo, hi))
        x, y = int(rng.integers(0, W - w)), int(rng.integers(0, H - h))
        b = np.array([x, y, x + w, y + h], dtype=F)
        if all(min(b[2], g[2]) <= max(b[0], g[0]) or min(b[3], g[3]) <= max(b[1], g[1]) for g in gts):
            gts.append(b)
    rows = []
    for v in views:
        x0, y0, cw, ch = v["crop"]
        full = (cw, ch) == (W, H)
        c = np.array([x0, y0, x0 + cw, y0 + ch], dtype=F)
        mine = []
        for g in gts:
            b = np.array([max(g[0], c[0]), max(g[1], c[1]), min(g[2], c[2]), min(g[3], c[3])], dtype=F)
            if b[2] <= b[0] or b[3] <= b[1]:
                continue
            vis = float((b[2] - b[0]) * (b[3] - b[1])) / float((g[2] - g[0]) * (g[3] - g[1]))
            if vis < visible:
                continue
            u = float(rng.uniform())
            score = full_score[0] + full_score[1] * u if full else 0.3 + 0.6 * vis * (0.8 + 0.2 * u)
            mine.append((b, score, 0))
        rows.append(mine)
    table = [dict(v, source=0, flip=k in flipped) for k, v in enumerate(views)]
    return build_pool(table, rows, max(1, max(len(r) for r in rows))), np.asarray(gts, dtype=F).reshape(-1, 4), (H, W)
