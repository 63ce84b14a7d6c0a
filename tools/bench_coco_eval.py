"""Cost of the on-device COCO bbox evaluation (sylph_amd.coco_eval.DeviceCOCOEvaluator) on a synthetic, COCO-val-sized set:
--images 5000 images, --categories 80, about --gt-per-image 7 boxes and --dets-per-image 100 detections per image.  Four detections in
five are a ground-truth box of their image, jittered; the rest are random.  Scores are random fp32.  --skew S moves that share of the
boxes to category 1 (a 'person'-like segment: one long chain of scan chunks for each of the category's blocks).

The rows are what process() would have appended, in batches of 192 images ((n, 8) fp32 device tensors); building them is not timed.
Per round (--rounds 3, after one warm-up round):
  evaluate     DeviceCOCOEvaluator.evaluate(), wall clock around it with a device synchronisation on both sides: the two sorts and the
               segment tables (torch), both kernels, the copy of the three result arrays and the summary means
  order        the torch plumbing alone (DeviceCOCOEvaluator._order), wall clock
  coco_match_kernel / coco_accumulate_kernel   the two launches, device time from sylph_profile_read_kernels
The yardstick (--yardstick) is the numpy restatement tests/cocoeval_ref.py on the same host, threads capped at 16, once: it is NOT pycocotools,
and nothing here says anything about pycocotools' speed.  With it the three arrays are also compared bit for bit.

One JSON line.
    python tools/bench_coco_eval.py --rounds 3 --yardstick
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "sylph-few-shot-detection_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
for _v in ("OMP_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(_v, "16")

import numpy as np  # noqa: E402
import torch  # noqa: E402


def synthetic_set(images, categories, gt_per_image, dets_per_image, seed=0, skew=0.0):
    """-> (COCO ground-truth dict, (images * dets_per_image, 8) fp32 rows in image order); skew: the share of boxes and of random detections
    that is moved to category 1 (COCO's 'person' holds about a third of val2017's boxes: one long segment for one block)"""
    rng = np.random.default_rng(seed)
    n_gt = rng.poisson(gt_per_image, images)
    anns, rows = [], []
    for i in range(images):
        g = int(n_gt[i])
        wh = np.exp(rng.uniform(np.log(8), np.log(300), (g, 2)))
        xy = rng.uniform(0, 500, (g, 2))
        cat = rng.integers(1, categories + 1, g)
        cat[rng.random(g) < skew] = 1
        crowd = rng.random(g) < 0.02
        for j in range(g):
            anns.append({"id": len(anns) + 1, "image_id": i + 1, "category_id": int(cat[j]), "bbox": [float(xy[j, 0]), float(xy[j, 1]), float(wh[j, 0]), float(wh[j, 1])],
                         "area": float(wh[j, 0] * wh[j, 1] * rng.uniform(0.4, 1.0)), "iscrowd": int(crowd[j])})
        d = dets_per_image
        box = np.concatenate([rng.uniform(0, 500, (d, 2)), np.exp(rng.uniform(np.log(8), np.log(300), (d, 2)))], axis=1)
        cls = rng.integers(0, categories, d)
        cls[rng.random(d) < skew] = 0
        if g:
            src = rng.integers(0, g, d)
            near = rng.random(d) < 0.8
            jit = np.concatenate([xy[src] + rng.normal(0, 0.08, (d, 2)) * wh[src], wh[src] * np.exp(rng.normal(0, 0.1, (d, 2)))], axis=1)
            box[near] = jit[near]
            cls[near] = cat[src][near] - 1
        r = np.zeros((d, 8), dtype=np.float32)
        r[:, 0] = i + 1
        r[:, 1:3] = box[:, :2]
        r[:, 3:5] = box[:, :2] + box[:, 2:]
        r[:, 5] = rng.random(d)
        r[:, 6] = cls
        r[:, 7] = 1
        rows.append(r)
    gt = {"images": [{"id": i + 1} for i in range(images)], "annotations": anns,
          "categories": [{"id": c + 1, "name": f"cat{c + 1}"} for c in range(categories)]}
    return gt, np.concatenate(rows)


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "rounds": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--categories", type=int, default=80)
    ap.add_argument("--gt-per-image", type=float, default=7.0)
    ap.add_argument("--dets-per-image", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skew", type=float, default=0.0, help="share of the boxes moved to category 1")
    ap.add_argument("--yardstick", action="store_true", help="also run tests/cocoeval_ref.py once and compare bit for bit")
    a = ap.parse_args()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from sylph_amd.coco_eval import DeviceCOCOEvaluator
    from sylph_amd.engine import Engine
    from sylph_amd.evaluation import detection_rows_to_coco

    gt, rows = synthetic_set(a.images, a.categories, a.gt_per_image, a.dets_per_image, skew=a.skew)
    eng = Engine(None, dtype="f32")
    c2d = {c: c + 1 for c in range(a.categories)}
    ev = DeviceCOCOEvaluator(gt, contiguous_to_dataset_id=c2d, engine=eng)
    per = 192 * a.dets_per_image
    batches = [torch.from_numpy(rows[i:i + per]).cuda() for i in range(0, len(rows), per)]
    res = {"images": a.images, "categories": a.categories, "ground_truth": len(gt["annotations"]), "detections": int(rows.shape[0]), "skew": a.skew,
           "detections_of_category_1": int((rows[:, 6] == 0).sum()),
           "max_gt_per_pair": ev._gt_host["max_per_pair"]}

    def once():
        ev.reset()
        ev._rows = list(batches)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ev.evaluate()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    once()  # warm-up: table upload, allocator, kernel load
    walls, match, acc, order = [], [], [], []
    for _ in range(a.rounds):
        ms, out = once()  # wall clock with the profile off
        walls.append(ms)
        eng.profile_enable(True)
        eng.profile_read()
        once()
        k = eng.profile_read()["kernels"]
        eng.profile_enable(False)
        match.append(k["coco_match_kernel"]["ms"])
        acc.append(k["coco_accumulate_kernel"]["ms"])
        allrows = torch.cat(batches)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev._order(allrows)
        torch.cuda.synchronize()
        order.append((time.perf_counter() - t0) * 1e3)
    res.update(evaluate=summary(walls), order=summary(order), coco_match_kernel=summary(match), coco_accumulate_kernel=summary(acc))
    res["bbox"] = {k: out["bbox"][k] for k in list(out["bbox"])[:12]}
    if a.yardstick:
        import cocoeval_ref as CR
        coco = detection_rows_to_coco(torch.from_numpy(rows), c2d)
        t0 = time.perf_counter()
        want_ev, want = CR.results(gt, coco)
        res["numpy_restatement_ms"] = (time.perf_counter() - t0) * 1e3
        bits = lambda x: np.ascontiguousarray(x).view(np.int64)
        res["bit_equal"] = {n: bool(np.array_equal(bits(getattr(ev, n)), bits(want_ev[n]))) for n in ("precision", "recall", "scores")}
        res["summary_equal"] = all((np.isnan(v) and np.isnan(out["bbox"][k])) or v == out["bbox"][k] for k, v in want.items())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
