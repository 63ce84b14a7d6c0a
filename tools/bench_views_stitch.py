"""Cost of the stitching view merge (sylph_stitch_views) next to the work in front of it and next to the large merge: the protocol and
the pool of tools/bench_views_large.py -- bf16, R-50-FPN, 5-way, synthetic weights, a pinned 8000 x 10000 source under 800 x 800
tiles at 20 % overlap plus the full frame (209 views, 41 800 pool rows).

Legs, each a child process; the driver alternates them --rounds times (>= 3):
  steps   the PARENT commit (--parent-tree: a checkout of it with a build of its own): the view steps preprocess_views -> backbone ->
          head -> decode_rows of the whole view list, timed per pass -> mean time of one step
  merge   this checkout: the same view list through the same steps once, then on its rows Engine.stitch_views (stitch_thr 0.5,
          border_px 2.0) and Engine.merge_views_large; both again on 8 sources x 20 full-frame views x 200 synthetic rows, where no
          row is cut; Engine.stitch_views on a one-class pool of 262 144 rows with K = 0 (no cut row either: one serial walk)
Times as in bench_views_large.py: `device_ms` the span of the entry's launches on the stream, `call_ms` the host clock around the
Engine call with its one read-back.  The condition: a stitch call costs less than the parent's mean view step.

    python tools/bench_views_stitch.py --parent-tree DIR --rounds 3 --repeats 5 [--out profiles/views_stitch_bench.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from bench_views_large import BIG_HW, OVERLAP, TILE, synthetic_rows, time_merge  # noqa: E402

TAG = "BENCH_VIEWS_STITCH_CHILD "
MERGE_KEYS = ("stitch_big", "large_merge_big", "stitch_8x20x200_no_cut", "large_merge_8x20x200", "stitch_one_class_262144")


def child(args):
    sys.path.insert(0, args.tree)
    sys.path.insert(0, os.path.join(args.tree, "sylph-few-shot-detection_amd"))
    import torch
    from sylph_amd import synthetic as Wt
    from sylph_amd import views as V
    from sylph_amd.runner import MetaFCOSRunner, create_cfg
    r = MetaFCOSRunner()
    cfg = create_cfg(r.get_default_cfg(), "sylph://COCO-Detection/Meta-FCOS/Meta-FCOS-finetune.yaml")
    model = r.build_model(cfg, dtype="bf16")
    model.load_state_dict(Wt.synthetic_state_dict(0, depth=50))
    model.eval()
    eng = model.engine
    codes = {k: v.cuda() for k, v in Wt.synthetic_codes(5, seed=100, scale=3.0).items()}
    h, w = BIG_HW
    g = torch.Generator().manual_seed(7)
    src = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).pin_memory()
    views = V.tile_views(h, w, TILE, OVERLAP, 800, 1333)
    table = [dict(v, source=0) for v in views]
    steps = V.plan_view_steps(table, V.DEFAULT_MAX_BATCH)
    table = [table[i] for st in steps for i in st]

    def run_steps():
        dev_src = [src.to("cuda", non_blocking=True)]
        rows = eng.new_view_rows(len(table))
        row0 = 0
        for st in steps:
            vs = table[row0:row0 + len(st)]
            eng.preprocess_views(dev_src, vs, rgb_input=False)
            eng.backbone()
            eng.head(codes["cls_conv"], codes["cls_bias"])
            eng.decode_rows(rows, row0, [V.view_out_size(v) for v in vs])
            row0 += len(st)
        return rows

    res = {"leg": args.leg, "tree": os.path.abspath(args.tree), "views": len(table), "steps": len(steps), "rows": len(table) * eng.default_max_out()}
    if args.leg == "steps":
        for _ in range(args.warmup):
            run_steps()
        ms = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_steps()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        res["steps_ms"] = ms
    else:
        rows = run_steps()
        res["rows_decoded"] = int(rows["counts"].sum().item())
        both = synthetic_rows(torch, 8, 20, 200, 5, 1000, 1)
        res["stitch_big"] = time_merge(torch, eng, lambda: eng.stitch_views(table, rows, [BIG_HW]), "stitch_kernels", args.repeats)
        out = eng.stitch_views(table, rows, [BIG_HW])[0]
        res["stitch_big"]["stitched_rows"] = int(out["stitched"].sum().item())
        res["large_merge_big"] = time_merge(torch, eng, lambda: eng.merge_views_large(table, rows), "merge_large_kernels", args.repeats)
        res["stitch_8x20x200_no_cut"] = time_merge(torch, eng, lambda: eng.stitch_views(both[0], both[1], [(1000, 1000)] * 8, max_out=400),
                                                   "stitch_kernels", args.repeats)
        res["large_merge_8x20x200"] = time_merge(torch, eng, lambda: eng.merge_views_large(both[0], both[1], max_out=400), "merge_large_kernels",
                                                 args.repeats)
        one = synthetic_rows(torch, 1, 1024, 256, 1, 8000, 2)
        res["stitch_one_class_262144"] = time_merge(torch, eng, lambda: eng.stitch_views(one[0], one[1], [(8000, 8000)], max_out=262144, topk=0),
                                                    "stitch_kernels", 1)
    print(TAG + json.dumps(res), flush=True)


def driver(args):
    if args.rounds < 3:
        raise SystemExit("--rounds must be at least 3")
    if not args.parent_tree or not os.path.isdir(args.parent_tree):
        raise SystemExit("--parent-tree: a built checkout of the parent commit is the yardstick")
    runs = {"steps": [], "merge": []}
    for rnd in range(args.rounds):
        for leg in ("steps", "merge"):  # alternating, each in a fresh process
            tree = os.path.abspath(args.parent_tree) if leg == "steps" else ROOT
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--tree", tree, "--repeats", str(args.repeats), "--warmup", str(args.warmup)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout)
            line = [l for l in p.stdout.splitlines() if l.startswith(TAG)]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"{leg} child of round {rnd} failed with {p.returncode}")
            runs[leg].append(json.loads(line[-1][len(TAG):]))
            print(f"round {rnd} {leg} done", file=sys.stderr, flush=True)
    passes = [m for r in runs["steps"] for m in r["steps_ms"]]
    n_steps = runs["steps"][0]["steps"]
    med = lambda key, field: statistics.median(r[key][field] for r in runs["merge"])
    out = {"views": runs["steps"][0]["views"], "steps": n_steps, "rows": runs["steps"][0]["rows"], "rows_decoded": runs["merge"][0]["rows_decoded"],
           "parent_steps_ms": {"min": min(passes), "median": statistics.median(passes), "max": max(passes), "passes": len(passes)},
           "parent_mean_step_ms": statistics.median(passes) / n_steps}
    for key in MERGE_KEYS:
        out[key] = {"device_ms": med(key, "device_ms"), "call_ms": med(key, "call_ms"), "rows_out": runs["merge"][0][key]["rows_out"]}
    out["stitch_big"]["stitched_rows"] = runs["merge"][0]["stitch_big"]["stitched_rows"]
    out["stitch_over_large_merge"] = out["stitch_big"]["device_ms"] / out["large_merge_big"]["device_ms"]
    out["stitch_below_one_step"] = out["stitch_big"]["call_ms"] < out["parent_mean_step_ms"]
    text = json.dumps(out) + "\n" + "\n".join(json.dumps(r) for leg in ("steps", "merge") for r in runs[leg]) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["steps", "merge"], default=None, help="child mode: one leg in this process")
    ap.add_argument("--tree", default=ROOT, help="child mode: the checkout whose sylph_amd package and library run the leg")
    ap.add_argument("--parent-tree", default=None, help="driver: a checkout of the parent commit, built, for the steps leg")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--child-timeout", type=int, default=420)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.leg:
        child(args)
    else:
        driver(args)


if __name__ == "__main__":
    main()
