"""Cost of MODEL.FCOS.USE_DEFORMABLE in the FCOS head (bf16, 800x1333 padded to 800x1344, random pyramid).

For each batch size, a plain and a deformable head are run on the same pyramid; per step (`head` = both towers, the prediction pass and
the class-conditional conv of a 5-way episode) it prints the whole-step time (HIP events) and the per-kernel times of the launches the
library times itself: in a head-only step `conv_igemm_kernel` is the 27-channel offset conv, `conv_deform_kernel` the deformable conv,
`conv_hpipe_kernel<true>` the plain GroupNorm-in tower layers.  The GroupNorm apply pass that the deformable layer's input needs is not
a conv launch: take it from a `rocprofv3 --kernel-trace --stats` run of this script (gn_apply_partials_kernel).

    python tools/bench_deform.py --batches 8 192 --steps 5
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "sylph-few-shot-detection_amd"))

import torch  # noqa: E402

LEVELS = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]


def cfg_for(deformable):
    from sylph_amd.config import get_default_cfg
    cfg = get_default_cfg()
    cg = cfg.MODEL.META_LEARN.CODE_GENERATOR
    cfg.MODEL.META_LEARN.EPISODIC_LEARNING = True
    cg.CONV_L2_NORM = True
    cg.TOWER_LAYERS = [["GN", "ReLU"], ["GN", "ReLU"]]
    cg.CLS_LAYER = ["", "", 1]
    cg.BIAS_LAYER = ["", "", 1]
    cfg.MODEL.FCOS.USE_DEFORMABLE = deformable
    return cfg


def run(B, deformable, steps, warmup):
    from sylph_amd import synthetic as Wt
    from sylph_amd.engine import Engine
    eng = Engine(cfg_for(deformable), dtype="bf16")
    eng.load_state_dict(Wt.head_state_dict(seed=3, deformable=deformable))
    g = torch.Generator(device="cuda").manual_seed(5)
    feats = [torch.randn(1, 256, h, w, generator=g, device="cuda").repeat(B, 1, 1, 1) for h, w in LEVELS]
    eng.import_pyramid(feats, (800, 1344), image_sizes=[(800, 1333)] * B)
    del feats
    codes = Wt.synthetic_codes(5, seed=4, scale=3.0)
    for _ in range(warmup):
        eng.head(codes["cls_conv"], codes["cls_bias"])
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        eng.head(codes["cls_conv"], codes["cls_bias"])
    b.record()
    torch.cuda.synchronize()
    step_ms = a.elapsed_time(b) / steps
    eng.profile_enable(True)
    eng.profile_read()
    for _ in range(steps):
        eng.head(codes["cls_conv"], codes["cls_bias"])
    torch.cuda.synchronize()
    kern = eng.profile_read()["kernels"]
    eng.profile_enable(False)
    per = {k: {"ms_per_launch": v["ms"] / max(1, v["launches"]), "launches_per_step": v["launches"] / steps,
               "tflops": v["flops"] / (v["ms"] * 1e-3) / 1e12 if v["ms"] > 0 else 0.0} for k, v in kern.items()}
    eng.close()
    return {"batch": B, "deformable": deformable, "head_ms_per_step": step_ms, "kernels": per}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 192])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only-deformable", action="store_true", help="one deformable run per batch (for a kernel trace)")
    args = ap.parse_args()
    for B in args.batches:
        for d in ([True] if args.only_deformable else [False, True]):
            print(json.dumps(run(B, d, args.steps, args.warmup)), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
