"""Cost and gain of a mixed-episode query step (sylph_fcos_head_episodes), bf16, R-50 head, 800x1333 padded to 800x1344.

Leg 1, head + decode on a random pyramid (HIP events around `head` / `head_episodes` + `decode`): B images of 5-way episodes, one
uniform step (`head`, one code set for the batch: the path that existed before) against mixed steps with E episodes (image i in episode
i % E).  The legs alternate inside every repeat; per leg the median, min and max over the repeats are printed, and the uniform leg's
max - min is the run-to-run spread a mixed leg is judged against.

Leg 2, the whole query step on synthetic images resident on the device (`preprocess` + `backbone` + head + `decode`, R-50 synthetic
weights): one mixed B-image step with B episodes against B batch-1 steps, one per episode (the reference's query loop,
meta_learn_evaluation.py:421-426).

One JSON line.  For per-kernel times run it under `rocprofv3 --kernel-trace --stats` (a run of its own).

    python tools/bench_mixed_episodes.py --batch 192 --episodes 1 8 48 192 --repeats 5 --steps 5
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

LEVELS = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]


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


def episode_codes(n):
    from sylph_amd import synthetic as Wt
    out = []
    for e in range(n):
        c = Wt.synthetic_codes(5, seed=100 + e, scale=3.0)
        out.append((c["cls_conv"].cuda(), c["cls_bias"].cuda()))
    return out


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats": len(ms)}


def head_decode_legs(B, episodes, repeats, steps, warmup):
    from sylph_amd import synthetic as Wt
    from sylph_amd.engine import Engine
    eng = Engine(cfg_episodic(), dtype="bf16")
    eng.load_state_dict(Wt.head_state_dict(seed=3))
    g = torch.Generator(device="cuda").manual_seed(5)
    feats = [torch.randn(4, 256, h, w, generator=g, device="cuda").repeat((B + 3) // 4, 1, 1, 1)[:B].contiguous() for h, w in LEVELS]
    eng.import_pyramid(feats, (800, 1344), image_sizes=[(800, 1333)] * B)
    del feats
    codes = episode_codes(max(episodes))
    legs = {"uniform": lambda: (eng.head(*codes[0]), eng.decode())}
    for E in episodes:
        ie = [i % E for i in range(B)]
        legs[f"mixed_E{E}"] = (lambda cs, ie: lambda: (eng.head_episodes(cs, ie), eng.decode()))(codes[:E], ie)
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():  # alternating: every leg once per repeat
            ms[k].append(timed(fn, steps))
    eng.close()
    out = {k: summary(v) for k, v in ms.items()}
    spread = out["uniform"]["max_ms"] - out["uniform"]["min_ms"]
    for k, v in out.items():
        if k != "uniform":
            v["median_minus_uniform_ms"] = v["median_ms"] - out["uniform"]["median_ms"]
            v["within_uniform_spread"] = abs(v["median_minus_uniform_ms"]) <= spread
    return {"batch": B, "ways": 5, "steps_per_repeat": steps, "uniform_spread_ms": spread, "legs": out}


def whole_step_legs(B, repeats, warmup):
    from sylph_amd import synthetic as Wt
    from sylph_amd.engine import Engine
    eng = Engine(cfg_episodic(), dtype="bf16")
    eng.load_state_dict(Wt.synthetic_state_dict(0, depth=50))
    base = [im.cuda() for im in Wt.synthetic_images(4, 800, 1333, seed=9)]
    images = [base[i % 4] for i in range(B)]
    codes = episode_codes(B)
    ie = list(range(B))

    def mixed():
        eng.preprocess(images)
        eng.backbone()
        eng.head_episodes(codes, ie)
        return eng.decode()

    def one_by_one():
        for i in range(B):
            eng.preprocess(images[i:i + 1])
            eng.backbone()
            eng.head(*codes[i])
            eng.decode()

    legs = {"mixed_one_step": mixed, "batch1_steps": one_by_one}
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            ms[k].append(timed(fn, 1))
    eng.close()
    out = {k: summary(v) for k, v in ms.items()}
    for v in out.values():
        v["img_per_s"] = B / (v["median_ms"] * 1e-3)
    return {"batch": B, "episodes": B, "legs": out, "batch1_over_mixed": out["batch1_steps"]["median_ms"] / out["mixed_one_step"]["median_ms"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=192)
    ap.add_argument("--episodes", type=int, nargs="+", default=[1, 8, 48, 192])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-whole-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mixed_episodes.py needs a GPU")
    res = {"head_decode": head_decode_legs(args.batch, [e for e in args.episodes if e <= args.batch], args.repeats, args.steps, args.warmup)}
    torch.cuda.empty_cache()
    if not args.skip_whole_step:
        res["whole_step"] = whole_step_legs(args.batch, args.repeats, args.warmup)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
