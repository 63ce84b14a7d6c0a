"""The COCO bbox protocol (evaluate -> accumulate -> summarize, useCats = 1) restated in plain float64 numpy / Python from the published
algorithm: the yardstick of sylph_amd.coco_eval.DeviceCOCOEvaluator.  Every operation that reaches a result is one IEEE float64 add, multiply,
divide or compare, in the order written here, so the device arrays can be compared bit for bit.

evaluate(gt, dets): gt is a COCO dict ("images", "annotations", "categories"), dets the list detection_rows_to_coco returns
({"image_id", "category_id", "bbox" XYWH, "score"}), in arrival order."""
from collections import OrderedDict, defaultdict

import numpy as np

IOU_THRS = np.linspace(.5, .95, 10)
REC_THRS = np.linspace(0, 1, 101)
AREA_RNGS = [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]
AREA_NAMES = ["all", "small", "medium", "large"]


def iou(d, g, crowd):
    """d, g: XYWH; crowd: the union is the detection's area"""
    iw = min(d[0] + d[2], g[0] + g[2]) - max(d[0], g[0])
    ih = min(d[1] + d[3], g[1] + g[3]) - max(d[1], g[1])
    if iw <= 0 or ih <= 0:
        return 0.0
    i = iw * ih
    u = d[2] * d[3] if crowd else d[2] * d[3] + g[2] * g[3] - i
    return i / u


def evaluate_pair(gts, dts, area_rng, max_det):
    """one (image, category) pair in one area range: dts are ordered by score and cut already.  -> None when the pair does not exist, else
    (matched [T, D] bool, ignored [T, D] bool, scores [D], non-ignored ground-truth count)"""
    if len(gts) == 0 and len(dts) == 0:
        return None
    g_ig = [bool(g.get("iscrowd", 0)) or g["area"] < area_rng[0] or g["area"] > area_rng[1] for g in gts]
    order = [i for i, x in enumerate(g_ig) if not x] + [i for i, x in enumerate(g_ig) if x]  # non-ignored first, each in original order
    ious = [[iou(d["bbox"], g["bbox"], bool(g.get("iscrowd", 0))) for g in gts] for d in dts]
    T, D = len(IOU_THRS), len(dts)
    matched = np.zeros((T, D), dtype=bool)
    ignored = np.zeros((T, D), dtype=bool)
    for ti, t in enumerate(IOU_THRS):
        taken = [False] * len(gts)
        for di, d in enumerate(dts):
            best = min(t, 1 - 1e-10)
            m = -1
            for gi in order:
                if taken[gi] and not gts[gi].get("iscrowd", 0):
                    continue
                if m > -1 and not g_ig[m] and g_ig[gi]:
                    break
                if ious[di][gi] < best:
                    continue
                best = ious[di][gi]
                m = gi
            if m > -1:
                taken[m] = True
                matched[ti, di] = True
                ignored[ti, di] = g_ig[m]
            else:
                a = d["bbox"][2] * d["bbox"][3]
                ignored[ti, di] = a < area_rng[0] or a > area_rng[1]
    return matched, ignored, np.array([d["score"] for d in dts], dtype=np.float64), sum(1 for x in g_ig if not x)


def evaluate(gt, dets, max_dets=(1, 10, 100), cat_ids=None):
    """-> {"precision" [T, R, K, A, M], "recall" [T, K, A, M], "scores" [T, R, K, A, M]} float64, -1 where a cell has no non-ignored ground truth"""
    img_ids = sorted(im["id"] for im in gt["images"])
    cat_ids = sorted(c["id"] for c in gt["categories"]) if cat_ids is None else sorted(cat_ids)
    known = set(img_ids)
    gts, dts = defaultdict(list), defaultdict(list)
    for g in gt["annotations"]:
        gts[g["image_id"], g["category_id"]].append(g)
    for d in dets:
        if d["image_id"] not in known:
            raise ValueError(f"detection on image id {d['image_id']}, which the ground truth does not hold")
        dts[d["image_id"], d["category_id"]].append(d)
    for key, ds in dts.items():
        idx = np.argsort([-d["score"] for d in ds], kind="mergesort")  # score descending, stable in arrival order
        dts[key] = [ds[i] for i in idx[:max_dets[-1]]]
    T, R, K, A, M = len(IOU_THRS), len(REC_THRS), len(cat_ids), len(AREA_RNGS), len(max_dets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    for k, cat in enumerate(cat_ids):
        for a, rng in enumerate(AREA_RNGS):
            pairs = [evaluate_pair(gts.get((im, cat), []), dts.get((im, cat), []), rng, max_dets[-1]) for im in img_ids]
            pairs = [p for p in pairs if p is not None]
            if not pairs:
                continue
            npig = sum(p[3] for p in pairs)
            if npig == 0:
                continue
            for m, md in enumerate(max_dets):
                sc = np.concatenate([p[2][:md] for p in pairs])
                inds = np.argsort(-sc, kind="mergesort")
                sc = sc[inds]
                dtm = np.concatenate([p[0][:, :md] for p in pairs], axis=1)[:, inds]
                dti = np.concatenate([p[1][:, :md] for p in pairs], axis=1)[:, inds]
                tps = np.cumsum(np.logical_and(dtm, np.logical_not(dti)), axis=1).astype(np.float64)
                fps = np.cumsum(np.logical_and(np.logical_not(dtm), np.logical_not(dti)), axis=1).astype(np.float64)
                for t in range(T):
                    tp, fp = tps[t], fps[t]
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    for i in range(nd - 1, 0, -1):  # non-increasing from the right
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    q, ss = np.zeros(R), np.zeros(R)
                    for ri, pi in enumerate(np.searchsorted(rc, REC_THRS, side="left")):
                        if pi < nd:
                            q[ri] = pr[pi]
                            ss[ri] = sc[pi]
                    precision[t, :, k, a, m] = q
                    scores[t, :, k, a, m] = ss
    return {"precision": precision, "recall": recall, "scores": scores}


def _mean(s):
    s = s[s > -1]
    return float(np.mean(s)) if s.size else -1.0


def twelve(precision, recall, max_dets=(1, 10, 100), ksel=slice(None)):
    """the COCO summary numbers of the category slice ksel, as fractions (-1: no entry): AP, AP50, AP75, APs, APm, APl, AR@maxDets.., ARs, ARm, ARl"""
    p, r = precision[:, :, ksel], recall[:, ksel]
    out = OrderedDict()
    out["AP"] = _mean(p[:, :, :, 0, -1])
    out["AP50"] = _mean(p[0, :, :, 0, -1])
    out["AP75"] = _mean(p[5, :, :, 0, -1])
    for a, n in ((1, "s"), (2, "m"), (3, "l")):
        out["AP" + n] = _mean(p[:, :, :, a, -1])
    for m, md in enumerate(max_dets):
        out[f"AR@{md}"] = _mean(r[:, :, 0, m])
    for a, n in ((1, "s"), (2, "m"), (3, "l")):
        out["AR" + n] = _mean(r[:, :, a, -1])
    return out


def results(gt, dets, max_dets=(1, 10, 100), category_subsets=None):
    """the "bbox" dict: the twelve numbers x 100 (NaN for -1), AP-<name> per category, and the twelve again per subset under the subset
    name's first letter ("novel" -> nAP, nAP50, ...)"""
    ev = evaluate(gt, dets, max_dets)
    cats = sorted(gt["categories"], key=lambda c: c["id"])
    pct = lambda v: v * 100 if v >= 0 else float("nan")
    out = OrderedDict((k, pct(v)) for k, v in twelve(ev["precision"], ev["recall"], max_dets).items())
    for k, c in enumerate(cats):
        out["AP-" + c["name"]] = pct(_mean(ev["precision"][:, :, k, 0, -1]))
    for name, ids in (category_subsets or {}).items():
        sub = evaluate(gt, dets, max_dets, cat_ids=ids)  # the subset's categories alone
        for key, v in twelve(sub["precision"], sub["recall"], max_dets).items():
            out[name[0] + key] = pct(v)
    return ev, out
