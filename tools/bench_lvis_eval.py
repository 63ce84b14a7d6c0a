"""Cost of the on-device LVIS bbox evaluation (sylph_amd.lvis_eval.DeviceLVISEvaluator) on a synthetic, LVIS-val-sized set:
--images 19809 images, --categories 1203, about --gt-per-image 12.4 boxes (245 000) whose categories follow a 1 / rank long tail, per
image a few negative and not exhaustively annotated categories, and --dets-per-image 300 detections (5.9 M rows).  Three detections in
five are a ground-truth box of their image, jittered; one in five is of one of the image's negative categories; the rest are random
(most of those are dropped by the federated filter).  Scores are random fp32.

The rows are what process() would have appended, in batches of 192 images ((n, 8) fp32 device tensors); building them is not timed.
Per round (--rounds 3, after one warm-up round):
  evaluate     evaluate(), wall clock around it with a device synchronisation on both sides
  order        the torch plumbing alone (_order), wall clock
  the launches' device time from sylph_profile_read_kernels (the accumulate runs once per slab of 256 categories; the sum is reported)
--protocol coco runs DeviceCOCOEvaluator(max_dets=(300,)) on the same rows and boxes instead: another protocol (no budget per image, no
federated filter, no ignore flags) over the same data through the dense images x categories pair table -- a yardstick for time only.
--tree DIR imports sylph_amd (and its library) from another checkout, e.g. the parent commit's.
--restatement-images N also evaluates the first N images alone, on the device and with tests/lviseval_ref.py (a numpy restatement of the
protocol, NOT lvis-api), and compares precision and recall bit for bit.

One JSON line.
    python tools/bench_lvis_eval.py --rounds 3 --restatement-images 300
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _v in ("OMP_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(_v, "16")

import numpy as np  # noqa: E402


def synthetic_set(images, categories, gt_per_image, dets_per_image, seed=0):
    """-> (LVIS ground-truth dict, (images * dets_per_image, 8) fp32 rows in image order, class c = category c + 1)"""
    rng = np.random.default_rng(seed)
    tail = 1.0 / np.arange(1, categories + 1)
    tail /= tail.sum()
    n_gt = rng.poisson(gt_per_image, images)
    anns, rows, imgs = [], [], []
    for i in range(images):
        g = int(n_gt[i])
        wh = np.exp(rng.uniform(np.log(8), np.log(300), (g, 2)))
        xy = rng.uniform(0, 500, (g, 2))
        cat = rng.choice(categories, g, p=tail) + 1
        ign = rng.random(g) < 0.02
        for j in range(g):
            anns.append({"id": len(anns) + 1, "image_id": i + 1, "category_id": int(cat[j]), "bbox": [float(xy[j, 0]), float(xy[j, 1]), float(wh[j, 0]), float(wh[j, 1])],
                         "area": float(wh[j, 0] * wh[j, 1] * rng.uniform(0.4, 1.0)), "ignore": int(ign[j])})
        pos = set(cat.tolist())
        neg = [int(c) for c in rng.choice(categories, 4, p=tail) + 1 if c not in pos]
        nel = [int(c) for c in pos if rng.random() < 0.15]
        imgs.append({"id": i + 1, "neg_category_ids": sorted(set(neg)), "not_exhaustive_category_ids": nel})
        d = dets_per_image
        box = np.concatenate([rng.uniform(0, 500, (d, 2)), np.exp(rng.uniform(np.log(8), np.log(300), (d, 2)))], axis=1)
        cls = rng.integers(0, categories, d)
        u = rng.random(d)
        if neg:
            cls[u > 0.8] = rng.choice(neg, int((u > 0.8).sum())) - 1
        if g:
            src = rng.integers(0, g, d)
            near = u < 0.6
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
    freq = lambda k: "f" if k < categories // 3 else ("c" if k < 2 * categories // 3 else "r")  # the head of the tail is frequent
    gt = {"images": imgs, "annotations": anns, "categories": [{"id": c + 1, "name": f"cat{c + 1}", "frequency": freq(c)} for c in range(categories)]}
    return gt, np.concatenate(rows)


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "rounds": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=19809)
    ap.add_argument("--categories", type=int, default=1203)
    ap.add_argument("--gt-per-image", type=float, default=12.4)
    ap.add_argument("--dets-per-image", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--protocol", choices=("lvis", "coco"), default="lvis")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose sylph_amd and library run (default: this one)")
    ap.add_argument("--restatement-images", type=int, default=0, help="compare the first N images bit for bit with tests/lviseval_ref.py")
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    sys.path[:0] = [tree, os.path.join(tree, "sylph-few-shot-detection_amd"), os.path.join(ROOT, "tests")]
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from sylph_amd.engine import Engine
    from sylph_amd.evaluation import detection_rows_to_coco

    gt, rows = synthetic_set(a.images, a.categories, a.gt_per_image, a.dets_per_image)
    eng = Engine(None, dtype="f32")
    c2d = {c: c + 1 for c in range(a.categories)}
    if a.protocol == "lvis":
        from sylph_amd.lvis_eval import DeviceLVISEvaluator
        make = lambda g: DeviceLVISEvaluator(g, contiguous_to_dataset_id=c2d, engine=eng)
        kernels = ("lvis_match_kernel", "coco_accumulate_kernel")
    else:
        from sylph_amd.coco_eval import DeviceCOCOEvaluator
        make = lambda g: DeviceCOCOEvaluator(g, contiguous_to_dataset_id=c2d, max_dets=(a.dets_per_image,), engine=eng)
        kernels = ("coco_match_kernel", "coco_accumulate_kernel")
    ev = make(gt)
    per = 192 * a.dets_per_image
    batches = [torch.from_numpy(rows[i:i + per]).cuda() for i in range(0, len(rows), per)]
    res = {"protocol": a.protocol, "tree": os.path.relpath(tree, ROOT), "images": a.images, "categories": a.categories, "ground_truth": len(gt["annotations"]),
           "detections": int(rows.shape[0]), "max_gt_per_pair": ev._gt_host["max_per_pair"]}

    def once():
        ev.reset()
        ev._rows = list(batches)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ev.evaluate()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    once()  # warm-up: table upload, allocator, kernel load
    walls, k0, k1, order = [], [], [], []
    for _ in range(a.rounds):
        ms, out = once()  # wall clock with the profile off
        walls.append(ms)
        eng.profile_enable(True)
        eng.profile_read()
        once()
        k = eng.profile_read()["kernels"]
        eng.profile_enable(False)
        k0.append(k[kernels[0]]["ms"])
        k1.append(k[kernels[1]]["ms"])
        allrows = torch.cat(batches)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        prep = ev._order(allrows)
        torch.cuda.synchronize()
        order.append((time.perf_counter() - t0) * 1e3)
    res.update({"evaluate": summary(walls), "order": summary(order), kernels[0]: summary(k0), kernels[1]: summary(k1)})
    if a.protocol == "lvis":
        used = prep["pairs"]["det_off"][int(prep["pairs"]["n"])]
        res.update(live_pairs=int(prep["pairs"]["n"]), pair_list_capacity=int(prep["pairs"]["cat"].numel()), rows_used=int(used))
    res["peak_device_MiB"] = torch.cuda.max_memory_allocated() / 2 ** 20
    res["bbox"] = {k: out["bbox"][k] for k in list(out["bbox"])[:9]}
    if a.restatement_images and a.protocol == "lvis":
        import lviseval_ref as LR
        n = a.restatement_images
        sub = {"images": gt["images"][:n], "annotations": [x for x in gt["annotations"] if x["image_id"] <= n], "categories": gt["categories"]}
        sub_rows = torch.from_numpy(rows[:n * a.dets_per_image])
        small = make(sub)
        small._rows = [sub_rows.cuda()]
        got = small.evaluate()
        dets = detection_rows_to_coco(sub_rows, c2d)
        pairs = {(x["image_id"], x["category_id"]) for x in sub["annotations"]} | {(d["image_id"], d["category_id"]) for d in dets}
        t0 = time.perf_counter()
        want_ev, want = LR.results(sub, dets, pairs=sorted(pairs))
        bits = lambda x: np.ascontiguousarray(x).view(np.int64)
        res["restatement"] = {"images": n, "detections": len(dets), "ground_truth": len(sub["annotations"]), "seconds": time.perf_counter() - t0,
                              "bit_equal": {m: bool(np.array_equal(bits(getattr(small, m)), bits(want_ev[m]))) for m in ("precision", "recall")},
                              "summary_equal": all((np.isnan(v) and np.isnan(got["bbox"][k])) or v == got["bbox"][k] for k, v in want.items()),
                              "AP": want["AP"]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
