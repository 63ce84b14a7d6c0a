"""Cost and gain of a code-sets query step (sylph_fcos_head_codesets + sylph_decode_nms_codesets): B images scored against G code sets,
bf16, R-50-FPN synthetic weights, 800x1333 padded to 800x1344 (the protocol of tools/bench_mixed_episodes.py).

Per G two legs, each a full query step through the model API from the same batch of images:
  fused    model(batch, class_code_sets=[d_0 .. d_{G-1}])         one backbone / tower pass, the class-conditional conv + decode per set
  uniform  [model(batch, class_code=d_g) for g in range(G)]       G whole steps: the path that existed before (the yardstick)
The legs alternate inside every repeat; per leg the median, min and max over the repeats are printed.  The yardstick's max - min at
G = 1 is the run-to-run spread a claim is judged against.  `--images host` (default) hands the model pinned host images, as a loader
does: every step uploads its batch, so the uniform leg uploads it G times; `--images device` keeps them resident.
Also reported: the marginal cost of a set, (t_fused(G) - t_fused(1)) / (G - 1), next to the class-conditional kernel (profile) and
decode (HIP events) time of one uniform step.

One JSON line.
    python tools/bench_code_sets.py --batch 192 --sets 1 2 5 10 --ways 5 --repeats 3
    python tools/bench_code_sets.py --batch 192 --sets 5 --ways 20 --repeats 3
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

import torch  # noqa: E402


def build_model():
    from sylph_amd import synthetic as Wt
    from sylph_amd.runner import MetaFCOSRunner, create_cfg
    r = MetaFCOSRunner()
    cfg = create_cfg(r.get_default_cfg(), "sylph://COCO-Detection/Meta-FCOS/Meta-FCOS-finetune.yaml")
    model = r.build_model(cfg, dtype="bf16")
    model.load_state_dict(Wt.synthetic_state_dict(0, depth=50))
    model.eval()
    return model


def code_sets(G, ways):
    from sylph_amd import synthetic as Wt
    return [{k: v.cuda() for k, v in Wt.synthetic_codes(ways, seed=100 + g, scale=3.0 if ways <= 8 else 2.5).items()} for g in range(G)]


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=192)
    ap.add_argument("--sets", type=int, nargs="+", default=[1, 2, 5, 10])
    ap.add_argument("--ways", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--images", choices=["host", "device"], default="host")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_code_sets.py needs a GPU")
    from sylph_amd import synthetic as Wt
    model = build_model()
    base = Wt.synthetic_images(4, 800, 1333, seed=9)
    base = [im.cuda() if args.images == "device" else im.pin_memory() for im in base]
    batch = [{"image": base[i % 4], "height": 800, "width": 1333} for i in range(args.batch)]
    sets = code_sets(max(args.sets), args.ways)
    kw = dict(run_type="meta_learn_test_instance")
    legs = {}
    for G in args.sets:
        legs[f"fused_G{G}"] = (lambda cs: lambda: model(batch, class_code_sets=cs, **kw))(sets[:G])
        legs[f"uniform_G{G}"] = (lambda cs: lambda: [model(batch, class_code=d, **kw) for d in cs])(sets[:G])
    for fn in legs.values():
        for _ in range(args.warmup):
            fn()
    ms = {k: [] for k in legs}
    for _ in range(args.repeats):
        for k, fn in legs.items():  # alternating: every leg once per repeat
            ms[k].append(wall(fn))
    out = {k: summary(v) for k, v in ms.items()}
    res = {"batch": args.batch, "ways": args.ways, "images": args.images, "legs": out, "per_G": {}}
    for G in args.sets:
        f, u = out[f"fused_G{G}"], out[f"uniform_G{G}"]
        row = {"fused_img_sets_per_s": args.batch * G / (f["median_ms"] * 1e-3), "uniform_img_sets_per_s": args.batch * G / (u["median_ms"] * 1e-3),
               "uniform_over_fused": u["median_ms"] / f["median_ms"], "uniform_spread_ms": u["max_ms"] - u["min_ms"],
               "fused_wins_beyond_spread": u["median_ms"] - f["median_ms"] > u["max_ms"] - u["min_ms"]}
        if G > 1 and 1 in args.sets:
            row["marginal_ms_per_set"] = (f["median_ms"] - out["fused_G1"]["median_ms"]) / (G - 1)
        res["per_G"][str(G)] = row
    # one uniform step's own class-conditional + decode time on the batch the last step left resident
    eng = model.engine
    w, b = sets[0]["cls_conv"], sets[0]["cls_bias"]
    eng.profile_enable(True)
    eng.profile_read()
    eng.head(w, b)
    torch.cuda.synchronize()
    kern = eng.profile_read()["kernels"]
    eng.profile_enable(False)
    cond = {n: v["ms"] for n, v in kern.items() if n in ("gn_logits_kernel", "logits_scan_kernel")}
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    eng.decode()
    a.record()
    for _ in range(5):
        eng.decode()
    e.record()
    torch.cuda.synchronize()
    res["uniform_step"] = {"class_conditional_kernel_ms": cond, "decode_ms": a.elapsed_time(e) / 5}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
