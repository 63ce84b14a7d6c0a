"""A shot sweep from a shot bank against fresh support passes, bf16, R-50-FPN, synthetic weights, 800x1333 support images.

The pool: 20 classes x 30 annotated instances on 60 images (10 boxes per image, the classes interleaved so that a class's instances
sit on 30 different images).  The sweep: K in {1, 2, 3, 5, 10, 30} shots per class x 10 seeds = 60 draws (ShotBank.draw).  Two legs
compute the class codes of the same draws:
  bank   evaluation.build_shot_bank over the pool ONCE (timed apart: bank_build_ms), then per draw ONE Engine.combine_shots call
  fresh  per draw: preprocess + backbone of the images that carry the draw's instances, then ONE codegen_rois call over them -- the
         yardstick: what a seed costs without a bank (already at one backbone pass per image, not per instance).  The batch is
         filled up to a multiple of 5 images with images of the pool that carry no drawn instance: a draw's image count varies
         (17 .. 60), and without the filling every draw met a batch shape whose plan had been evicted and paid its rebuild (a first
         run measured 117 - 350 ms per draw with spreads of 35 - 125 ms at K <= 10 against 16.5 ms at K = 30, where every draw has
         60 images); with it the sweep has eight batch shapes and the yardstick is steady, at up to four images of extra work
The legs alternate for 3 rounds (bank, fresh, bank, fresh, ...); a round of a leg runs all 60 draws.  Per K the output has the mean
per-draw time of each leg and round, and the summary the yardstick's spread over its rounds next to the difference between the legs.
A draw is timed with the host synchronised before and after (wall clock), so the bank leg includes its table upload and launch
latency.  max_code_diff_over_max compares the legs' codes: the per-shot rows of a 600-ROI call and of a K x 20-ROI call may come from
different conv routes whose fp32 sums differ in their last bits before the tower's bf16 stores, so this is of the order of a bf16 ulp
(2^-8), not zero (tests/test_shot_bank_gpu.py pins the equal-route identity).

Prints one JSON line per (K, leg, round) and per K, and writes them to profiles/shot_bank_bench.txt.

    python tools/bench_shot_bank.py
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "sylph-few-shot-detection_amd"))

import torch  # noqa: E402

from bench_support_rois import instance_boxes  # noqa: E402

CLASSES, PER_CLASS, PER_IMAGE = 20, 30, 10
SHOTS = [1, 2, 3, 5, 10, 30]


def pool_records():
    """60 records of 800x1333 with 10 boxes each; instance i of image b has class (b * 10 + i) % 20: 30 instances per class"""
    from sylph_amd import synthetic as Wt
    from sylph_amd.structures import Boxes, Instances
    n_img = CLASSES * PER_CLASS // PER_IMAGE
    base = [im.cuda() for im in Wt.synthetic_images(4, 800, 1333, seed=9)]
    boxes = instance_boxes(n_img * PER_IMAGE, seed=3)
    recs = []
    for b in range(n_img):
        inst = Instances((800, 1333))
        inst.gt_boxes = Boxes(boxes[b * PER_IMAGE:(b + 1) * PER_IMAGE])
        inst.gt_classes = torch.tensor([(b * PER_IMAGE + i) % CLASSES for i in range(PER_IMAGE)])
        recs.append({"image": base[b % 4], "instances": inst, "height": 800, "width": 1333, "image_id": b})
    return recs


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch-step", type=int, default=5, help="the fresh leg's batches are filled up to a multiple of this many images")
    ap.add_argument("--images-per-item", type=int, default=20, help="images per build_shot_bank batch")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shot_bank_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_shot_bank.py needs a GPU")
    from sylph_amd import synthetic as Wt
    from sylph_amd.evaluation import build_shot_bank
    from sylph_amd.runner import MetaFCOSRunner, create_cfg
    runner = MetaFCOSRunner()
    cfg = create_cfg(runner.get_default_cfg(), "sylph://COCO-Detection/Meta-FCOS/Meta-FCOS-finetune.yaml")
    model = runner.build_model(cfg, dtype="bf16")
    model.load_state_dict(Wt.synthetic_state_dict(0, depth=50))
    model.eval()
    eng = model.engine
    recs = pool_records()
    n = args.images_per_item
    loader = [recs[i:i + n] for i in range(0, len(recs), n)]
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    build_shot_bank(model, loader)  # warm: plans built, clocks up
    build_ms, bank = wall_ms(lambda: build_shot_bank(model, loader))
    assert len(bank) == CLASSES * PER_CLASS and all(len(bank.rows_of(c)) == PER_CLASS for c in range(CLASSES))
    rows = bank.tensor()
    emit({"bank_build_ms": round(build_ms, 2), "instances": len(bank), "images": len(recs), "bank_bytes": bank.nbytes,
          "bank_bytes_per_instance": bank.nbytes // len(bank), "instances_per_s": round(len(bank) / (build_ms * 1e-3), 1)})
    all_boxes = torch.cat([r["instances"].gt_boxes.tensor for r in recs]).cuda()  # row r of the bank is instance r of the pool
    draws = {K: [bank.draw(K, seed) for seed in range(args.seeds)] for K in SHOTS}

    def from_bank(draw):
        idx, seg_len, _ = draw
        return eng.combine_shots(rows, idx, seg_len)[0]

    def fresh(draw):
        idx, seg_len, _ = draw
        imgs = sorted({bank.image_ids[r] for r in idx})
        spare = [b for b in range(len(recs)) if b not in set(imgs)]
        imgs += spare[:-len(imgs) % args.batch_step]  # (see the module docstring: few batch shapes, plans stay cached)
        slot = {b: i for i, b in enumerate(imgs)}
        eng.preprocess([recs[b]["image"] for b in imgs])
        eng.backbone()
        return eng.codegen_rois(all_boxes[idx], [slot[bank.image_ids[r]] for r in idx], seg_len)

    legs = {"bank": from_bank, "fresh": fresh}
    diff = {}
    for K in SHOTS:  # warm-up: every plan and support pass of the sweep built before anything is timed
        for d in draws[K]:
            a, b = from_bank(d).float(), fresh(d).float()
            diff[K] = max(diff.get(K, 0.0), float((a - b).abs().max()) / float(b.abs().max()))
    ms = {K: {name: [] for name in legs} for K in SHOTS}
    for rnd in range(args.rounds):
        for name, fn in legs.items():  # alternating: every leg once per round
            for K in SHOTS:
                t = sum(wall_ms(lambda: fn(d))[0] for d in draws[K]) / len(draws[K])
                ms[K][name].append(t)
                emit({"K": K, "leg": name, "round": rnd, "draws": len(draws[K]), "ms_per_draw": round(t, 3)})
    for K in SHOTS:
        mean = {name: sum(v) / len(v) for name, v in ms[K].items()}
        emit({"K": K, "summary": True, "bank_ms_per_draw": round(mean["bank"], 3), "fresh_ms_per_draw": round(mean["fresh"], 3),
              "speedup": round(mean["fresh"] / mean["bank"], 1), "bank_spread_ms": round(max(ms[K]["bank"]) - min(ms[K]["bank"]), 3),
              "fresh_spread_ms": round(max(ms[K]["fresh"]) - min(ms[K]["fresh"]), 3), "bank_below_fresh_min": bool(max(ms[K]["bank"]) < min(ms[K]["fresh"])),
              "max_code_diff_over_max": round(diff[K], 6)})
    total = {name: sum(sum(ms[K][name]) / len(ms[K][name]) * len(draws[K]) for K in SHOTS) for name in legs}
    emit({"sweep": True, "draws": sum(len(v) for v in draws.values()), "bank_sweep_ms": round(total["bank"], 1), "bank_build_ms": round(build_ms, 1),
          "fresh_sweep_ms": round(total["fresh"], 1), "speedup_with_build": round(total["fresh"] / (total["bank"] + build_ms), 2)})
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
