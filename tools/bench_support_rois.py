"""Support throughput from ROI lists (sylph_codegen_rois) against one backbone pass per instance, bf16, R-50, synthetic weights.

B support images of 800x1333 carry k annotated boxes each (k = 1, 4, 11), grouped into classes of 5 shots.  Two legs compute the
same B * k / 5 class codes from the same instances:
  rois       one step = preprocess + backbone of the B images, then ONE codegen_rois call over the R = B * k (image, box) pairs
  duplicate  one step = preprocess + backbone of a batch that repeats each image k times (image r of it = the image of instance r),
             then codegen_classes(boxes, 5): what a caller had to do before, the backbone run once per instance
The legs alternate inside one process and each runs twice (rois, duplicate, rois, duplicate), so the spread of a leg between its own
two runs is visible next to the difference between the legs.  At k = 1 both legs launch the same work: the rois leg is expected to lie
within the duplicate leg's own spread (printed as within_duplicate_spread).

Prints one line per (k, leg, run) and one summary line per k, and writes them to profiles/support_rois_bench.txt.  For per-kernel
times run it under `rocprofv3 --kernel-trace --stats` (a run of its own).

    python tools/bench_support_rois.py --images 20 --boxes 1 4 11 --steps 50
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "sylph-few-shot-detection_amd"))

import torch  # noqa: E402

SHOTS = 5


def cfg_episodic():
    from sylph_amd.config import get_default_cfg
    cfg = get_default_cfg()
    cg = cfg.MODEL.META_LEARN.CODE_GENERATOR
    cfg.MODEL.META_LEARN.EPISODIC_LEARNING = True
    cg.CONV_L2_NORM = True
    cg.TOWER_LAYERS = [["GN", "ReLU"], ["GN", "ReLU"]]
    cg.CLS_LAYER = ["", "", 1]
    cg.BIAS_LAYER = ["", "", 1]
    return cfg


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def instance_boxes(R, seed):
    """R boxes inside an 800x1333 image whose sizes spread over the pyramid levels."""
    g = torch.Generator().manual_seed(seed)
    bw = 32 + torch.rand(R, generator=g) * 600
    bh = 32 + torch.rand(R, generator=g) * 500
    x0 = torch.rand(R, generator=g) * (1333 - bw)
    y0 = torch.rand(R, generator=g) * (800 - bh)
    return torch.stack([x0, y0, x0 + bw, y0 + bh], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=20, help="B: distinct support images (B * k must be a multiple of 5)")
    ap.add_argument("--boxes", type=int, nargs="+", default=[1, 4, 11], help="k: annotated boxes per image")
    ap.add_argument("--steps", type=int, default=50, help="steps per timed run (a k = 1 step is 6 ms: 50 steps time 0.3 s)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "support_rois_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_support_rois.py needs a GPU")
    from sylph_amd import synthetic as Wt
    from sylph_amd.engine import Engine
    eng = Engine(cfg_episodic(), dtype="bf16")
    eng.load_state_dict(Wt.synthetic_state_dict(0, depth=50))
    B = args.images
    base = [im.cuda() for im in Wt.synthetic_images(4, 800, 1333, seed=9)]
    images = [base[i % 4] for i in range(B)]
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    for k in args.boxes:
        R = B * k
        assert R % SHOTS == 0, f"{B} images x {k} boxes is not a whole number of {SHOTS}-shot classes"
        # instance r: box r on image r % B (every image has k instances, consecutive shots of a class sit on different images)
        roi_image = [r % B for r in range(R)]
        boxes = instance_boxes(R, seed=k).cuda()
        seg_len = [SHOTS] * (R // SHOTS)
        dup_images = [images[b] for b in roi_image]

        def rois():
            eng.preprocess(images)
            eng.backbone()
            return eng.codegen_rois(boxes, roi_image, seg_len)

        def duplicate():
            eng.preprocess(dup_images)
            eng.backbone()
            return eng.codegen_classes(boxes, SHOTS)

        legs = {"rois": rois, "duplicate": duplicate}
        for _ in range(args.warmup):  # alternating like the timed runs: both plans built, clocks up before the first timed leg
            for fn in legs.values():
                fn()
        a, b = rois().float(), duplicate().float()
        scale = float(b.abs().max())
        torch.cuda.synchronize()
        ms = {name: [] for name in legs}
        for run in range(2):
            for name, fn in legs.items():  # alternating: every leg once per run
                t = timed(fn, args.steps)
                ms[name].append(t)
                emit({"k": k, "images": B, "instances": R, "classes": R // SHOTS, "leg": name, "run": run, "ms_per_step": round(t, 3),
                      "instances_per_s": round(R / (t * 1e-3), 1), "images_per_s": round(B / (t * 1e-3), 1),
                      "backbone_passes_per_step": B if name == "rois" else R})
        mean = {n: sum(v) / len(v) for n, v in ms.items()}
        spread = max(ms["duplicate"]) - min(ms["duplicate"])
        emit({"k": k, "summary": True, "rois_ms": round(mean["rois"], 3), "duplicate_ms": round(mean["duplicate"], 3),
              "speedup": round(mean["duplicate"] / mean["rois"], 2), "rois_spread_ms": round(max(ms["rois"]) - min(ms["rois"]), 3),
              "duplicate_spread_ms": round(spread, 3),
              "within_duplicate_spread": bool(min(ms["duplicate"]) <= mean["rois"] <= max(ms["duplicate"])) if k == 1 else None,
              "max_code_diff_over_max": round(float((a - b).abs().max()) / scale, 6)})
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
