"""Cost of fine-tuning class codes on query records (sylph_fcos_targets / sylph_cls_grad, sylph_amd.finetune).
bf16, R-50-FPN synthetic weights, 20-way 10-shot: 200 support images of 800x1333 (padded to 800x1344), one box each, stored once as
records of --record-batch images.  Per round (--rounds, default 3), every leg once, alternating; per leg the median, min and max:

  targets          load_record + Engine.fcos_targets per record (wall)
  grad_20 / _80    load_record + Engine.cls_grad per record at N = 20 / 80 (wall), and the profiled device time of the launches of one
                   call (cls_grad_kernel + its partial sums; 1 resp. 3 class blocks)
  score_20         the yardstick: the scoring launch gn_logits_kernel at N = 20 on the same record (profiled device time, same build:
                   head_fused.hip is the parent's source under the parent's flags)
  steps            finetune_class_codes over all records per step, --steps steps: steps per second, and the time of 500 steps scaled
                   from it

One JSON line.
    python tools/bench_finetune.py --record-batch 8 --steps 50
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "sylph-few-shot-detection_amd"))

import torch  # noqa: E402

from bench_records import build_model, codes, wall  # noqa: E402


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "rounds": len(v)}


def kernel_ms(eng, fn, name):
    eng.profile_enable(True)
    eng.profile_read()
    fn()
    torch.cuda.synchronize()
    k = eng.profile_read()["kernels"]
    eng.profile_enable(False)
    return sum(v["ms"] for n, v in k.items() if n.startswith(name))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ways", type=int, default=20)
    ap.add_argument("--shots", type=int, default=10)
    ap.add_argument("--record-batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_finetune.py needs a GPU")
    from sylph_amd import synthetic as Wt
    from sylph_amd.finetune import finetune_class_codes
    model = build_model()
    eng = model.engine
    n_img = args.ways * args.shots
    base = [im.cuda() for im in Wt.synthetic_images(4, 800, 1333, seed=9)]
    boxes = Wt.synthetic_boxes(n_img, 800, 1333, seed=11)
    records, anns = [], []
    for i in range(0, n_img, args.record_batch):
        idx = list(range(i, min(n_img, i + args.record_batch)))
        r = model([{"image": base[j % 4], "height": 800, "width": 1333, "image_id": j} for j in idx], run_type="meta_learn_cache_query")[0]
        records.append(r["record"])
        anns.append({"boxes": boxes[idx], "classes": torch.tensor([j % args.ways for j in idx]), "image_index": torch.arange(len(idx))})
    d20, d80 = codes(args.ways, 200), codes(80, 300)
    targets = []
    for rec, a in zip(records, anns):
        eng.load_record(rec)
        targets.append(eng.fcos_targets(a["boxes"], a["classes"], a["image_index"]))

    def leg_targets():
        for rec, a in zip(records, anns):
            eng.load_record(rec)
            eng.fcos_targets(a["boxes"], a["classes"], a["image_index"])

    def leg_grad(d):
        def run():
            for rec, t in zip(records, targets):
                eng.load_record(rec)
                eng.cls_grad(t[0], d["cls_conv"], d["cls_bias"], check_labels=False)
        return run

    legs = {"targets": leg_targets, "grad_20": leg_grad(d20), "grad_80": leg_grad(d80),
            "steps": lambda: finetune_class_codes(eng, records, anns, d20, iters=args.steps, lr=0.01)}
    dev = {"grad_20": lambda: eng.cls_grad(targets[0][0], d20["cls_conv"], d20["cls_bias"], check_labels=False),
           "grad_80": lambda: eng.cls_grad(targets[0][0], d80["cls_conv"], d80["cls_bias"], check_labels=False),
           "score_20": lambda: eng.head(d20["cls_conv"], d20["cls_bias"])}
    dev_name = {"grad_20": "cls_grad", "grad_80": "cls_grad", "score_20": "gn_logits_kernel"}
    ms = {k: [] for k in legs}
    dms = {k: [] for k in dev}
    for it in range(1 + args.rounds):  # one warm-up round
        for k, fn in legs.items():
            t = wall(fn)
            if it:
                ms[k].append(t)
        for k, fn in dev.items():  # alternating: the yardstick and the two gradient calls once per round, on record 0
            eng.load_record(records[0])
            t = kernel_ms(eng, fn, dev_name[k])
            if it:
                dms[k].append(t)
    n = len(records)
    res = {"ways": args.ways, "shots": args.shots, "images": n_img, "records": n, "images_per_record": args.record_batch,
           "record_bytes_per_image": records[0].nbytes / records[0].batch[0],
           "per_record_wall_ms": {k: summary([t / n for t in ms[k]]) for k in ("targets", "grad_20", "grad_80")},
           "device_ms_record0": {k: summary(v) for k, v in dms.items()},
           "steps_per_second": summary([args.steps / (t / 1e3) for t in ms["steps"]]),
           "ms_500_steps": summary([t / args.steps * 500 for t in ms["steps"]])}
    s = res["device_ms_record0"]
    res["grad_20_over_score_20"] = s["grad_20"]["median"] / s["score_20"]["median"]
    res["grad_80_over_grad_20"] = s["grad_80"]["median"] / s["grad_20"]["median"]
    for rec in records:
        rec.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
