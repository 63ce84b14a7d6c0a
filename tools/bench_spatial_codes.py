"""Cost of a 3x3 class-conditional conv (CODE_GENERATOR.CLS_LAYER kernel size 3) in the query head, bf16, R-50 head, B images of
800x1333 padded to 800x1344, N classes.

Yardstick: the 3x3 classifier the library could already run -- `head_pretrained()` on a synthetic checkpoint whose cls_logits.weight
is (N, 256, 3, 3): the last cls GroupNorm apply pass, then one conv_igemm launch.  This leg uses nothing the feature adds (it runs
unchanged on a build that predates it, or on that build's library through SYLPH_LIB_PATH).
Feature: `head()` with (N, 256, 3, 3) codes on an engine configured for 3x3 codes: `head_3x3` is the default route (the apply +
conv_igemm on the packed codes), `head_3x3_fused` the same call with SYLPH_GN_COND3X3=1 (gn_cond3x3_kernel: GroupNorm + ReLU + conv
in one pass, N <= 32; the knob is read per call).  --generic (SYLPH_FUSE_GN_LOGITS=0, a run of its own: that knob is read once) also
un-fuses the prediction convs.
For information: `head()` with 1x1 codes on the yardstick engine (gn_logits_kernel).

Per leg: the call's time by HIP events (median / min / max over the repeats, the legs alternating inside every repeat; the yardstick
runs TWICE per repeat -- `pretrained_a`, `pretrained_b` -- and the distance of their medians is the spread a difference is judged
against), and the summed per-launch times of its class-conditional kernels from sylph_profile_read_kernels in a pass of its own.
The yardstick sum is `gn_apply_partials_kernel` + `conv_igemm_kernel` of the pretrained leg, both from the profile.  A library that
predates the apply's profile record gives no such row; the sum is then derived from the event times of the run:
    towers + prediction pass = head(1x1) - gn_logits_kernel
    apply + conv_igemm       = pretrained - (towers + prediction pass)

One JSON line.    python tools/bench_spatial_codes.py --batch 64 --ways 5 32 --repeats 5 --steps 5
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "sylph-few-shot-detection_amd"))

LEVELS = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]


def cfg_episodic(ksize):
    from sylph_amd.config import get_default_cfg
    cfg = get_default_cfg()
    cg = cfg.MODEL.META_LEARN.CODE_GENERATOR
    cfg.MODEL.META_LEARN.EPISODIC_LEARNING = True
    cg.CONV_L2_NORM = True
    cg.TOWER_LAYERS = [["GN", "ReLU"], ["GN", "ReLU"]]
    cg.CLS_LAYER = ["", "", ksize]
    cg.BIAS_LAYER = ["", "", 1]
    return cfg


def timed(fn, steps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats": len(ms)}


def kernel_ms(eng, fn, steps):
    """per-launch time of every profiled kernel of `fn` (a pass of its own: the event pairs serialise the launches)"""
    eng.profile_enable(True)
    eng.profile_read()
    for _ in range(steps):
        fn()
    k = eng.profile_read()["kernels"]
    eng.profile_enable(False)
    return {n: {"ms_per_launch": v["ms"] / max(v["launches"], 1), "launches_per_call": v["launches"] / steps} for n, v in k.items()}


def codes(n, k, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, 256, k, k, generator=g)
    w = w / w.flatten(1).norm(dim=1).view(n, 1, 1, 1) * 3.0
    return w.cuda(), torch.full((n,), -4.6).cuda()


def run(B, N, repeats, steps, warmup, generic, yardstick_only=False):
    import torch
    from sylph_amd import synthetic as Wt
    from sylph_amd.engine import Engine
    sd = Wt.head_state_dict(seed=3, num_classes=N)
    g = torch.Generator().manual_seed(17)
    sd["proposal_generator.fcos_head.cls_logits.weight"] = torch.randn(N, 256, 3, 3, generator=g) * 0.01
    gd = torch.Generator(device="cuda").manual_seed(5)
    feats = [torch.randn(4, 256, h, w, generator=gd, device="cuda").repeat((B + 3) // 4, 1, 1, 1)[:B].contiguous() for h, w in LEVELS]

    def engine(ksize):
        eng = Engine(cfg_episodic(ksize), dtype="bf16")
        eng.load_state_dict(sd)
        eng.import_pyramid(feats, (800, 1344), image_sizes=[(800, 1333)] * B)
        return eng

    legs, engines, kern = {}, {}, {}
    if not generic:
        e1 = engines["k1"] = engine(1)
        c1 = codes(N, 1, 40 + N)
        legs["pretrained_a"] = e1.head_pretrained
        legs["pretrained_b"] = e1.head_pretrained
        legs["head_1x1"] = lambda: e1.head(*c1)
    try:
        if not yardstick_only:
            e3 = engines["k3"] = engine(3)
            c3 = codes(N, 3, 50 + N)
            legs["head_3x3_generic" if generic else "head_3x3"] = lambda: e3.head(*c3)
            if not generic:
                def fused():
                    os.environ["SYLPH_GN_COND3X3"] = "1"
                    try:
                        e3.head(*c3)
                    finally:
                        del os.environ["SYLPH_GN_COND3X3"]
                legs["head_3x3_fused"] = fused
    except NotImplementedError as err:  # a build without the feature: the yardstick legs alone
        print(f"# 3x3 codes are not available in this build ({err})", file=sys.stderr)
    del feats
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            ms[k].append(timed(fn, steps))
    out = {"ways": N, "legs": {k: summary(v) for k, v in ms.items()}}
    if "k1" in engines:
        kern["pretrained"] = kernel_ms(engines["k1"], legs["pretrained_a"], steps)
        kern["head_1x1"] = kernel_ms(engines["k1"], legs["head_1x1"], steps)
    if "k3" in engines:
        for k, v in legs.items():
            if k.startswith("head_3x3"):
                kern[k] = kernel_ms(engines["k3"], v, steps)
    out["kernels"] = kern
    L = out["legs"]
    if "k1" in engines:
        med = lambda k: L[k]["median_ms"]
        pre = 0.5 * (med("pretrained_a") + med("pretrained_b"))
        conv = kern["pretrained"].get("conv_igemm_kernel", {}).get("ms_per_launch")
        gnl = kern["head_1x1"].get("gn_logits_kernel", {}).get("ms_per_launch")
        d = {"pretrained_spread_ms": abs(med("pretrained_a") - med("pretrained_b")), "conv_igemm_ms": conv, "gn_logits_ms": gnl}
        apply = kern["pretrained"].get("gn_apply_partials_kernel", {}).get("ms_per_launch")
        if conv is not None and apply is not None:
            d["apply_ms"], d["apply_plus_conv_igemm_ms"], d["yardstick_sum_from"] = apply, apply + conv, "profile"
        elif conv is not None and gnl is not None:
            d["towers_and_predictions_ms"] = med("head_1x1") - gnl
            d["apply_plus_conv_igemm_ms"] = pre - d["towers_and_predictions_ms"]
            d["apply_ms"], d["yardstick_sum_from"] = d["apply_plus_conv_igemm_ms"] - conv, "event times"
        if "head_3x3_fused" in L:
            fused = kern["head_3x3_fused"].get("gn_cond3x3_kernel", {}).get("ms_per_launch")
            d["gn_cond3x3_ms"] = fused
            d["pretrained_minus_head_3x3_ms"] = pre - med("head_3x3")
            d["pretrained_minus_head_3x3_fused_ms"] = pre - med("head_3x3_fused")
            if fused is not None and "apply_plus_conv_igemm_ms" in d:
                d["yardstick_sum_minus_fused_ms"] = d["apply_plus_conv_igemm_ms"] - fused
                d["fused_faster_by_more_than_spread"] = d["yardstick_sum_minus_fused_ms"] > d["pretrained_spread_ms"]
        out["derived"] = d
    for e in engines.values():
        e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--ways", type=int, nargs="+", default=[5, 32])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--yardstick-only", action="store_true", help="no 3x3 engine (a library of a build without the feature through SYLPH_LIB_PATH)")
    ap.add_argument("--generic", action="store_true", help="the conv route of the 3x3 head alone (sets SYLPH_FUSE_GN_LOGITS=0 for this process)")
    args = ap.parse_args()
    if args.generic:
        os.environ["SYLPH_FUSE_GN_LOGITS"] = "0"
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_spatial_codes.py needs a GPU")
    res = {"batch": args.batch, "steps_per_repeat": args.steps, "generic": args.generic, "library": os.environ.get("SYLPH_LIB_PATH", "product"),
           "cases": []}
    for n in args.ways:
        res["cases"].append(run(args.batch, n, args.repeats, args.steps, args.warmup, args.generic, args.yardstick_only))
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
