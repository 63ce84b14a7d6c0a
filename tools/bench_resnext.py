"""Cost of a ResNeXt backbone (bf16, X-101-32x8d: DEPTH 101, NUM_GROUPS 32, WIDTH_PER_GROUP 8, STRIDE_IN_1X1 False) in a 5-way 5-shot
query step at B = 1, 16 and 192 (preprocess + backbone + FPN + head + decode) on 800x1333 images padded to 800x1344, synthetic weights.

For each batch size it prints the whole-step time (HIP events, img/s) and the per-kernel times of the launches the library times itself;
for `conv_group_kernel` (the grouped 3x3 conv2 of every block) also the effective HBM rate on algorithmic bytes: each launch's input and
output activations plus its packed weights, read / written once.  Cross-check the kernel times with a separate
`rocprofv3 --kernel-trace --stats` run of this script.

    python tools/bench_resnext.py --batches 1 16 192 --steps 3
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "sylph-few-shot-detection_amd"))

import torch  # noqa: E402

DEPTH, GROUPS, WPG = 101, 32, 8
BLOCKS = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}


def cfg_for():
    from sylph_amd.config import get_default_cfg
    cfg = get_default_cfg()
    cg = cfg.MODEL.META_LEARN.CODE_GENERATOR
    cfg.MODEL.META_LEARN.EPISODIC_LEARNING = True
    cg.CONV_L2_NORM = True
    cg.TOWER_LAYERS = [["GN", "ReLU"], ["GN", "ReLU"]]
    cg.CLS_LAYER = ["", "", 1]
    cg.BIAS_LAYER = ["", "", 1]
    r = cfg.MODEL.RESNETS
    r.DEPTH, r.NUM_GROUPS, r.WIDTH_PER_GROUP, r.STRIDE_IN_1X1 = DEPTH, GROUPS, WPG, False
    return cfg


def grouped_bytes(B, H=800, W=1344):
    """Algorithmic bytes of all grouped launches of one step: bf16 input + output maps, bf16 weights (C x C/G x 9)."""
    h, w = (H - 1) // 2 + 1, (W - 1) // 2 + 1  # stem (stride 2), then the max-pool (stride 2)
    h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    total = 0
    for si, nb in enumerate(BLOCKS[DEPTH]):
        mid = (GROUPS * WPG) << si
        for bi in range(nb):
            s = 2 if (bi == 0 and si > 0) else 1
            ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
            total += 2 * B * mid * (h * w + ho * wo) + 2 * mid * (mid // GROUPS) * 9
            h, w = ho, wo
    return total


def run(B, steps, warmup):
    from sylph_amd import synthetic as Wt
    from sylph_amd.engine import Engine
    eng = Engine(cfg_for(), dtype="bf16")
    sd = Wt.backbone_state_dict(0, depth=DEPTH, num_groups=GROUPS, width_per_group=WPG)
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
    out = {"backbone": f"X-{DEPTH}-{GROUPS}x{WPG}d", "batch": B, "step_ms": step_ms, "img_per_s": B / (step_ms * 1e-3), "kernels": per}
    g = per.get("conv_group_kernel")
    if g:
        gb = grouped_bytes(B)
        out["conv_group"] = {"ms_per_step": g["ms_per_step"], "algorithmic_GB": gb / 1e9, "effective_TBps": gb / (g["ms_per_step"] * 1e-3) / 1e12}
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16, 192])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    for B in args.batches:
        print(json.dumps(run(B, args.steps, args.warmup)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
