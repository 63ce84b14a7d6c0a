"""References of the query-views path (tests/test_views_cpu.py, tests/test_views_gpu.py), CPU only.

* input: Pillow crop -> resize(BILINEAR) -> mirror, then the BGR swap, normalisation and padding of the network input, in float32
* merge: the seven rules of sylph_merge_views (include/sylph_hip.h), followed literally in float32 numpy; plus a brute-force O(n^2)
  restatement that shares no code with it
* draw_rows: synthetic per-view detection rows whose same-class IoUs keep a margin from the NMS threshold (checked here, on the CPU)
"""
from typing import Dict, List, Optional, Sequence

import numpy as np

F = np.float32


# ---- input ---------------------------------------------------------------------------------------------------------------------
def view_image(src: np.ndarray, view: Dict) -> np.ndarray:
    """(h, w, 3) uint8 source -> the view's uint8 image: crop, resize, mirror"""
    from PIL import Image, ImageOps
    x0, y0, cw, ch = view["crop"]
    nh, nw = view["size"]
    im = Image.fromarray(src).crop((x0, y0, x0 + cw, y0 + ch)).resize((nw, nh), Image.BILINEAR)
    if view.get("flip", False):
        im = ImageOps.mirror(im)
    return np.asarray(im)


def network_input(images: Sequence[np.ndarray], mean, std, rgb_input: bool, divisibility: int = 32) -> np.ndarray:
    """uint8 HWC images -> (B, 3, H, W) float32: BGR swap when the images are RGB, (x - mean) * (1 / std), zero padded to the largest
    image rounded up to `divisibility`"""
    H = max(im.shape[0] for im in images)
    W = max(im.shape[1] for im in images)
    H, W = (H + divisibility - 1) // divisibility * divisibility, (W + divisibility - 1) // divisibility * divisibility
    out = np.zeros((len(images), 3, H, W), dtype=F)
    m = np.asarray(mean, dtype=F)
    inv = (F(1) / np.asarray(std, dtype=F)).astype(F)
    for b, im in enumerate(images):
        px = im[:, :, ::-1] if rgb_input else im
        v = ((px.astype(F) - m[None, None, :]).astype(F) * inv[None, None, :]).astype(F)
        out[b, :, :im.shape[0], :im.shape[1]] = v.transpose(2, 0, 1)
    return out


def bf16_round(x: np.ndarray) -> np.ndarray:
    """float32 -> the nearest bfloat16 (ties to even), as float32"""
    u = np.ascontiguousarray(x, dtype=F).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(F)


# ---- merge ---------------------------------------------------------------------------------------------------------------------
def to_source(box: np.ndarray, view: Dict) -> np.ndarray:
    """rule 1: one (4,) float32 box of a view -> source coordinates"""
    x0, y0, cw = F(view["crop"][0]), F(view["crop"][1]), F(view["crop"][2])
    x1, y1, x2, y2 = F(box[0]), F(box[1]), F(box[2]), F(box[3])
    if view.get("flip", False):
        x1, x2 = F(cw - x2), F(cw - x1)
    return np.array([F(x1 + x0), F(y1 + y0), F(x2 + x0), F(y2 + y0)], dtype=F)


def _suppresses(a: np.ndarray, b: np.ndarray, thr: float) -> bool:
    """rule 4: does the kept box a suppress b (same class)?  inter / (area_a + area_b - inter) > thr, float32 throughout"""
    w = max(F(0), F(min(a[2], b[2]) - max(a[0], b[0])))
    h = max(F(0), F(min(a[3], b[3]) - max(a[1], b[1])))
    inter = F(w * h)
    area_a = F(F(a[2] - a[0]) * F(a[3] - a[1]))
    area_b = F(F(b[2] - b[0]) * F(b[3] - b[1]))
    with np.errstate(divide="ignore", invalid="ignore"):
        return bool(F(inter / F(F(area_a + area_b) - inter)) > F(thr))


def merge_ref(view_table: List[Dict], boxes: np.ndarray, scores: np.ndarray, classes: np.ndarray, counts: np.ndarray, n_src: int,
              thr: float, K: int, max_out: Optional[int] = None) -> List[Dict]:
    """view_table[v] = {"source", "crop", "flip"}; boxes [V][max_in][4], scores / classes [V][max_in], counts [V] -> per source
    {"pred_boxes", "scores", "pred_classes", "view_index", "view_row", "truncated"}"""
    out = []
    for s in range(n_src):
        # 2: the pool -- views ascending, rows in order; 1: in source coordinates
        pool = [(v, r) for v in range(len(view_table)) if view_table[v]["source"] == s for r in range(int(counts[v]))]
        pb = [to_source(boxes[v, r], view_table[v]) for v, r in pool]
        ps = [F(scores[v, r]) for v, r in pool]
        pc = [int(classes[v, r]) for v, r in pool]
        # 3: stable, score descending (the pool order is (view, row) ascending already)
        order = sorted(range(len(pool)), key=lambda i: -float(ps[i]))
        # 4: greedy class-aware NMS
        kept = []
        for i in order:
            if thr > 0 and any(pc[j] == pc[i] and _suppresses(pb[j], pb[i], thr) for j in kept):
                continue
            kept.append(i)
        # 5: the first K kept and every later kept box whose score equals the K-th
        if K > 0 and len(kept) > K:
            kth = ps[kept[K - 1]]
            kept = kept[:K] + [i for i in kept[K:] if ps[i] == kth]
        truncated = max_out is not None and len(kept) > max_out
        if truncated:
            kept = kept[:max_out]
        out.append({"pred_boxes": np.array([pb[i] for i in kept], dtype=F).reshape(-1, 4), "scores": np.array([ps[i] for i in kept], dtype=F),
                    "pred_classes": np.array([pc[i] for i in kept], dtype=np.int64),
                    "view_index": np.array([pool[i][0] for i in kept], dtype=np.int64),  # 6: provenance
                    "view_row": np.array([pool[i][1] for i in kept], dtype=np.int64), "truncated": truncated})
    return out


def merge_bruteforce(view_table, boxes, scores, classes, counts, n_src, thr, K):
    """The same result from the definition, without a greedy walk: with the pool in final order, box i is kept iff no KEPT box j < i of
    its class overlaps it -- resolved as a fixed point over the full n x n overlap matrix (vectorised float32)."""
    out = []
    V = len(view_table)
    for s in range(n_src):
        vr = np.array([(v, r) for v in range(V) if view_table[v]["source"] == s for r in range(int(counts[v]))], dtype=np.int64).reshape(-1, 2)
        n = len(vr)
        b = boxes[vr[:, 0], vr[:, 1]].astype(F).reshape(-1, 4).copy()
        for k, (v, _) in enumerate(vr):
            t = view_table[v]
            if t.get("flip", False):
                cw = F(t["crop"][2])
                b[k, 0], b[k, 2] = F(cw - b[k, 2]), F(cw - b[k, 0])
            b[k, 0::2] = (b[k, 0::2] + F(t["crop"][0])).astype(F)
            b[k, 1::2] = (b[k, 1::2] + F(t["crop"][1])).astype(F)
        sc = scores[vr[:, 0], vr[:, 1]].astype(F)
        cl = classes[vr[:, 0], vr[:, 1]].astype(np.int64)
        order = np.lexsort((vr[:, 1], vr[:, 0], -sc.astype(np.float64)))
        b, sc, cl, vr = b[order], sc[order], cl[order], vr[order]
        keep = np.ones(n, dtype=bool)
        if thr > 0 and n:
            area = ((b[:, 2] - b[:, 0]).astype(F) * (b[:, 3] - b[:, 1]).astype(F)).astype(F)
            w = np.maximum(F(0), (np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0])).astype(F))
            h = np.maximum(F(0), (np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1])).astype(F))
            inter = (w * h).astype(F)
            with np.errstate(divide="ignore", invalid="ignore"):
                iou = (inter / ((area[:, None] + area[None, :]).astype(F) - inter).astype(F)).astype(F)
            over = (iou > F(thr)) & (cl[:, None] == cl[None, :]) & (np.arange(n)[:, None] < np.arange(n)[None, :])  # [j, i]: j before i
            while True:  # kept(i) = not any_j (kept(j) and over[j, i]); the matrix is strictly upper triangular: at most n rounds
                new = ~(over & keep[:, None]).any(axis=0)
                if np.array_equal(new, keep):
                    break
                keep = new
        idx = np.nonzero(keep)[0]
        if K > 0 and len(idx) > K:
            idx = idx[sc[idx] >= sc[idx[K - 1]]]
        out.append({"pred_boxes": b[idx], "scores": sc[idx], "pred_classes": cl[idx], "view_index": vr[idx, 0], "view_row": vr[idx, 1]})
    return out


def min_iou_margin(view_table, boxes, scores, classes, counts, n_src, thr) -> float:
    """the smallest |IoU - thr| over the same-class pairs of every source's pool (float64 IoU of the float32 source boxes)"""
    best = np.inf
    for s in range(n_src):
        vr = [(v, r) for v in range(len(view_table)) if view_table[v]["source"] == s for r in range(int(counts[v]))]
        if len(vr) < 2:
            continue
        b = np.array([to_source(boxes[v, r], view_table[v]) for v, r in vr], dtype=np.float64)
        cl = np.array([classes[v, r] for v, r in vr])
        area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        w = np.maximum(0, np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0]))
        h = np.maximum(0, np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1]))
        inter = w * h
        iou = inter / (area[:, None] + area[None, :] - inter)
        m = (cl[:, None] == cl[None, :]) & ~np.eye(len(vr), dtype=bool)
        if m.any():
            best = min(best, float(np.abs(iou[m] - thr).min()))
    return best


def _ious64(b: np.ndarray, others: np.ndarray) -> np.ndarray:
    b = b.astype(np.float64)
    o = others.astype(np.float64)
    w = np.maximum(0, np.minimum(b[2], o[:, 2]) - np.maximum(b[0], o[:, 0]))
    h = np.maximum(0, np.minimum(b[3], o[:, 3]) - np.maximum(b[1], o[:, 1]))
    inter = w * h
    return inter / ((b[2] - b[0]) * (b[3] - b[1]) + (o[:, 2] - o[:, 0]) * (o[:, 3] - o[:, 1]) - inter)


def draw_rows(view_table: List[Dict], max_in: int, counts: Sequence[int], n_classes: int, seed: int, thr: float, score_levels: int = 0,
              margin: float = 1e-4, n_objects: int = 6):
    """Per-view rows for `merge`: boxes cluster around a few objects per source (so that views overlap and NMS has work), given in the
    view's own (possibly mirrored) crop coordinates; rows of a view in descending score order as decode leaves them.  score_levels > 0
    quantises the scores to that many values: equal scores across views and inside them.  The condition on the inputs -- every
    same-class pair of a source at least `margin` away from the NMS threshold in IoU -- is enforced while drawing (a box that breaks
    it is drawn again) and asserted on the result."""
    rng = np.random.RandomState(seed)
    V = len(view_table)
    boxes = np.zeros((V, max_in, 4), dtype=F)
    scores = np.zeros((V, max_in), dtype=F)
    classes = np.zeros((V, max_in), dtype=np.int32)
    n_src = max(t["source"] for t in view_table) + 1
    objs = [[(rng.uniform(20, 200), rng.uniform(20, 150), rng.uniform(20, 60), rng.uniform(20, 60), rng.randint(n_classes))
             for _ in range(n_objects)] for _ in range(n_src)]
    placed = [[np.zeros((0, 4), dtype=F) for _ in range(n_classes)] for _ in range(n_src)]  # source boxes so far, per class
    for v, t in enumerate(view_table):
        x0, y0, cw = t["crop"][0], t["crop"][1], t["crop"][2]
        n = int(counts[v])
        sc = rng.uniform(0.05, 1.0, size=n)
        if score_levels > 0:
            sc = np.floor(sc * score_levels) / score_levels + 0.01
        sc = np.sort(sc.astype(F))[::-1]
        for r in range(n):
            while True:
                cx, cy, w, h, c = objs[t["source"]][rng.randint(n_objects)]
                c = c if rng.rand() < 0.8 else rng.randint(n_classes)
                bx = np.array([cx - w / 2 + rng.uniform(-9, 9), cy - h / 2 + rng.uniform(-9, 9), cx + w / 2 + rng.uniform(-9, 9),
                               cy + h / 2 + rng.uniform(-9, 9)])
                bx[0::2] -= x0
                bx[1::2] -= y0
                if t.get("flip", False):
                    bx[0], bx[2] = cw - bx[2], cw - bx[0]
                bx = bx.astype(F)
                sb = to_source(bx, t)
                prev = placed[t["source"]][c]
                if len(prev) == 0 or np.abs(_ious64(sb, prev) - thr).min() >= 2 * margin:
                    break
            placed[t["source"]][c] = np.concatenate([prev, sb[None]])
            boxes[v, r] = bx
            classes[v, r] = c
        scores[v, :n] = sc
    cnt = np.asarray(counts, dtype=np.int32)
    got = min_iou_margin(view_table, boxes, scores, classes, cnt, n_src, thr)
    assert got >= margin, f"seed {seed}: a same-class pair's IoU is {got:.2e} from NMS_TH {thr}"
    return boxes, scores, classes, cnt
