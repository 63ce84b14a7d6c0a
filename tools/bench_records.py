"""Cost and gain of query records (sylph_record_store / sylph_record_load): class codes scored on stored tower outputs.
bf16, R-50-FPN synthetic weights, B images of 800x1333 padded to 800x1344, resident inputs (the protocol of tools/bench_code_sets.py).

Legs, all through the model API, alternating inside every repeat; per leg the median, min and max over the repeats:
  fresh            model(batch, class_code=5-way)                      the whole step: the yardstick, of the same build
  store            Engine.store_record() on the batch the fresh step left (the record is closed again outside the timing)
  score_5 / _20 / _60   model(records, class_code=N-way)               head + decode on the loaded record
  score_5x5        model(records, class_code_sets=five 5-way sets)
  sweep_fresh      ten 5-way code sets arriving one at a time, as ten fresh steps
  sweep_records    the same ten sets as ONE network pass (run_type "meta_learn_cache_query") + ten record scores (+ closing the record)
The fresh leg's max - min is the run-to-run spread a ratio is judged against.  Also reported: the record's bytes per image and the
profiled kernels of one 5-way record score (no tower or backbone launch).

One JSON line.
    python tools/bench_records.py --batch 192 --repeats 5
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


def codes(ways, seed):
    from sylph_amd import synthetic as Wt
    scale = 3.0 if ways <= 8 else (2.5 if ways <= 32 else 2.0)
    return {k: v.cuda() for k, v in Wt.synthetic_codes(ways, seed=seed, scale=scale).items()}


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
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_records.py needs a GPU")
    from sylph_amd import synthetic as Wt
    model = build_model()
    eng = model.engine
    base = [im.cuda() for im in Wt.synthetic_images(4, 800, 1333, seed=9)]
    batch = [{"image": base[i % 4], "height": 800, "width": 1333, "image_id": i} for i in range(args.batch)]
    d5, d20, d60 = codes(5, 100), codes(20, 200), codes(60, 300)
    ten = [codes(5, 100 + g) for g in range(10)]
    kw = dict(run_type="meta_learn_test_instance")
    records = model(batch, run_type="meta_learn_cache_query")
    rec = records[0]["record"]
    held = []

    def store():
        held.append(eng.store_record())

    def sweep_records():
        r = model(batch, run_type="meta_learn_cache_query")
        for d in ten:
            model(r, class_code=d, **kw)
        r[0]["record"].close()

    legs = {
        "fresh": lambda: model(batch, class_code=d5, **kw),
        "store": store,  # (follows the fresh leg: the batch it left is current)
        "score_5": lambda: model(records, class_code=d5, **kw),
        "score_20": lambda: model(records, class_code=d20, **kw),
        "score_60": lambda: model(records, class_code=d60, **kw),
        "score_5x5": lambda: model(records, class_code_sets=ten[:5], **kw),
        "sweep_fresh": lambda: [model(batch, class_code=d, **kw) for d in ten],
        "sweep_records": sweep_records,
    }
    ms = {k: [] for k in legs}
    for it in range(args.warmup + args.repeats):
        for k, fn in legs.items():  # alternating: every leg once per repeat
            t = wall(fn)
            if it >= args.warmup:
                ms[k].append(t)
            while held:
                held.pop().close()
    out = {k: summary(v) for k, v in ms.items()}
    fresh = out["fresh"]
    res = {"batch": args.batch, "legs": out, "fresh_spread_ms": fresh["max_ms"] - fresh["min_ms"],
           "record_bytes": rec.nbytes, "record_bytes_per_image": rec.nbytes / args.batch,
           "fresh_over_score": {k: fresh["median_ms"] / out[k]["median_ms"] for k in ("score_5", "score_20", "score_60")},
           "five_fresh_over_score_5x5": 5 * fresh["median_ms"] / out["score_5x5"]["median_ms"],
           "sweep_fresh_over_sweep_records": out["sweep_fresh"]["median_ms"] / out["sweep_records"]["median_ms"]}
    eng.profile_enable(True)
    eng.profile_read()
    model(records, class_code=d5, **kw)
    torch.cuda.synchronize()
    res["score_5_kernels"] = {n: {"launches": v["launches"], "ms": v["ms"]} for n, v in eng.profile_read()["kernels"].items()}
    eng.profile_enable(False)
    rec.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
