"""Cost of the BasicBlock backbones (bf16, R-18 and R-34: MODEL.RESNETS.DEPTH 18 | 34, RES2_OUT_CHANNELS 64) in a 5-way query step
at B = 1, 16 and 192 (preprocess + backbone + FPN + head + decode) on 800x1333 images padded to 800x1344, synthetic weights.

For each depth and batch size it prints one JSON line: the whole-step time (HIP events, img/s) and the per-kernel times of the launches
the library times itself; for `conv_rw64_kernel` (every res2 conv: 3x3, 64 -> 64) also its share of the MFMA peak (2.5 PFLOP/s dense
bf16) on shape-derived FLOPs and the effective HBM rate on algorithmic bytes: each launch's input and output activations, the
residual where there is one, and the weights, read / written once.  Cross-check the kernel times with a separate
`rocprofv3 --kernel-trace --stats` run of this script.

    python tools/bench_resnet_basic.py --batches 1 16 192 --steps 3 [--depths 18 34 50] [--out profiles/resnet_basic_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "sylph-few-shot-detection_amd"))

import torch  # noqa: E402

BLOCKS = {18: (2, 2, 2, 2), 34: (3, 4, 6, 3)}
MFMA_PEAK = 2.5e15  # dense bf16 FLOP/s


def cfg_for(depth):
    from sylph_amd.config import get_default_cfg
    cfg = get_default_cfg()
    cg = cfg.MODEL.META_LEARN.CODE_GENERATOR
    cfg.MODEL.META_LEARN.EPISODIC_LEARNING = True
    cg.CONV_L2_NORM = True
    cg.TOWER_LAYERS = [["GN", "ReLU"], ["GN", "ReLU"]]
    cg.CLS_LAYER = ["", "", 1]
    cg.BIAS_LAYER = ["", "", 1]
    r = cfg.MODEL.RESNETS
    r.DEPTH, r.RES2_OUT_CHANNELS = depth, 64 if depth in BLOCKS else 256  # (--depths 50: the bottleneck R-50 under the same protocol)
    return cfg


def conv64_bytes(depth, B, H=800, W=1344):
    """Algorithmic bytes of the res2 launches of one step: per conv the bf16 input and output maps and the weights; per block one more
    map, the residual conv2 adds."""
    h, w = (H - 1) // 2 + 1, (W - 1) // 2 + 1  # stem (stride 2), then the max-pool (stride 2)
    h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    amap = 2 * B * 64 * h * w
    return BLOCKS[depth][0] * (2 * (2 * amap + 2 * 64 * 64 * 9) + amap)


def run(depth, B, steps, warmup):
    from sylph_amd import synthetic as Wt
    from sylph_amd.engine import Engine
    eng = Engine(cfg_for(depth), dtype="bf16")
    sd = Wt.backbone_state_dict(0, depth=depth)
    sd.update(Wt.head_state_dict(1, num_classes=60))
    eng.load_state_dict(sd)
    four = Wt.synthetic_images(4, 800, 1333, seed=3)
    imgs = [four[i % 4] for i in range(B)]
    codes = Wt.synthetic_codes(5, seed=4, scale=3.0)

    def step():
        eng.preprocess(imgs)
        eng.backbone()
        eng.head(codes["cls_conv"], codes["cls_bias"])
        eng.decode()

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        step()
    b.record()
    torch.cuda.synchronize()
    step_ms = a.elapsed_time(b) / steps
    eng.profile_enable(True)
    eng.profile_read()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    kern = eng.profile_read()["kernels"]
    eng.profile_enable(False)
    per = {k: {"ms_per_step": v["ms"] / steps, "launches_per_step": v["launches"] / steps,
               "tflops": v["flops"] / (v["ms"] * 1e-3) / 1e12 if v["ms"] > 0 else 0.0} for k, v in kern.items()}
    out = {"backbone": f"R-{depth}", "batch": B, "step_ms": step_ms, "img_per_s": B / (step_ms * 1e-3), "kernels": per}
    g = per.get("conv_rw64_kernel")
    if g and depth in BLOCKS:
        gb = conv64_bytes(depth, B)
        out["conv_rw64"] = {"ms_per_step": g["ms_per_step"], "launches_per_step": g["launches_per_step"], "tflops": g["tflops"],
                            "mfma_peak_share": g["tflops"] * 1e12 / MFMA_PEAK, "algorithmic_GB": gb / 1e9,
                            "effective_TBps": gb / (g["ms_per_step"] * 1e-3) / 1e12}
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16, 192])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--depths", type=int, nargs="+", default=[18, 34])
    ap.add_argument("--out", default=None, help="also write the results as a JSON list to this file")
    args = ap.parse_args()
    results = []
    for depth in args.depths:
        for B in args.batches:
            results.append(run(depth, B, args.steps, args.warmup))
            print(json.dumps(results[-1]), flush=True)
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"protocol": f"bf16, 800x1333 images padded to 800x1344, 5 classes, preprocess + backbone + FPN + head + decode, "
                                   f"{args.warmup} warm-up + {args.steps} timed steps (HIP events), synthetic weights",
                       "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
