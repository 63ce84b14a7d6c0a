"""Reference of the large view merge (tests/test_views_large_cpu.py, tests/test_views_large_gpu.py), CPU only: the rules above
sylph_merge_views (include/sylph_hip.h) as one greedy walk in float32 numpy.  It loops over the sorted pool and compares each row with
the kept boxes of its class in one vectorised step, so pools of tens of thousands of rows take about a second.  It shares no code with
the library, nor with tests/views_ref.py, which the CPU test holds it against."""
from typing import Dict, List, Optional

import numpy as np

F = np.float32


def merge_large_ref(view_table: List[Dict], boxes: np.ndarray, scores: np.ndarray, classes: np.ndarray, counts: np.ndarray, n_src: int,
                    thr: float, K: int, max_out: Optional[int] = None) -> List[Dict]:
    """view_table[v] = {"source", "crop", "flip"}; boxes [V][max_in][4], scores / classes [V][max_in], counts [V] (a count outside
    [0, max_in] is clamped) -> per source {"pred_boxes", "scores", "pred_classes", "view_index", "view_row", "truncated", "kept"};
    "kept" is the number of rows NMS left, before rule 5 and max_out cut it."""
    max_in = scores.shape[1]
    thr32 = F(thr)
    out = []
    for s in range(n_src):
        vs = [v for v in range(len(view_table)) if view_table[v]["source"] == s]
        # rule 2: views ascending, rows in order
        n_rows = [min(max(int(counts[v]), 0), max_in) for v in vs]
        vi = np.repeat(np.asarray(vs, dtype=np.int64), n_rows)
        ri = np.concatenate([np.arange(n, dtype=np.int64) for n in n_rows]) if vs else np.zeros(0, dtype=np.int64)
        b = boxes[vi, ri].astype(F).reshape(-1, 4)
        # rule 1: flip, then offset
        flip = np.array([bool(view_table[v].get("flip", False)) for v in vi], dtype=bool)
        cw = np.array([view_table[v]["crop"][2] for v in vi], dtype=F)
        x0 = np.array([view_table[v]["crop"][0] for v in vi], dtype=F)
        y0 = np.array([view_table[v]["crop"][1] for v in vi], dtype=F)
        x1 = np.where(flip, (cw - b[:, 2]).astype(F), b[:, 0])
        x2 = np.where(flip, (cw - b[:, 0]).astype(F), b[:, 2])
        sb = np.stack([(x1 + x0).astype(F), (b[:, 1] + y0).astype(F), (x2 + x0).astype(F), (b[:, 3] + y0).astype(F)], axis=1).reshape(-1, 4)
        sc = scores[vi, ri].astype(F)
        cl = classes[vi, ri].astype(np.int64)
        # rule 3: stable
        order = np.argsort(-sc, kind="stable")
        area = ((sb[:, 2] - sb[:, 0]).astype(F) * (sb[:, 3] - sb[:, 1]).astype(F)).astype(F)
        # rule 4: greedy, against the kept boxes of the row's class
        per_class = {}  # class -> [boxes (cap, 4), areas (cap,), count]
        kept = []
        for i in order:
            if thr > 0:
                slot = per_class.get(cl[i])
                if slot is None:
                    slot = per_class[cl[i]] = [np.empty((16, 4), dtype=F), np.empty(16, dtype=F), 0]
                kb, ka, n = slot
                if n:
                    w = np.maximum(F(0), (np.minimum(kb[:n, 2], sb[i, 2]) - np.maximum(kb[:n, 0], sb[i, 0])).astype(F))
                    h = np.maximum(F(0), (np.minimum(kb[:n, 3], sb[i, 3]) - np.maximum(kb[:n, 1], sb[i, 1])).astype(F))
                    inter = (w * h).astype(F)
                    with np.errstate(divide="ignore", invalid="ignore"):
                        iou = (inter / ((ka[:n] + area[i]).astype(F) - inter).astype(F)).astype(F)
                    if bool((iou > thr32).any()):
                        continue
                if n == len(ka):
                    kb = slot[0] = np.concatenate([kb, np.empty_like(kb)])
                    ka = slot[1] = np.concatenate([ka, np.empty_like(ka)])
                kb[n] = sb[i]
                ka[n] = area[i]
                slot[2] = n + 1
            kept.append(i)
        kept = np.asarray(kept, dtype=np.int64)
        n_kept = len(kept)
        # rule 5
        if K > 0 and n_kept > K:
            kth = sc[kept[K - 1]]
            kept = np.concatenate([kept[:K], kept[K:][sc[kept[K:]] == kth]])
        truncated = max_out is not None and len(kept) > max_out
        if truncated:
            kept = kept[:max_out]
        out.append({"pred_boxes": sb[kept].reshape(-1, 4), "scores": sc[kept], "pred_classes": cl[kept], "view_index": vi[kept],
                    "view_row": ri[kept], "truncated": truncated, "kept": n_kept})
    return out
