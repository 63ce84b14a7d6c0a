"""Cost of the large view merge (sylph_merge_views_large) next to the work in front of it: bf16, R-50-FPN, 5-way, synthetic weights,
pinned host sources.

Legs, each a child process; the driver alternates them --rounds times (>= 3):
  steps   the PARENT commit (--parent-tree: a checkout of it with a build of its own): one 8000 x 10000 source, 800 x 800 tiles at
          20 % overlap plus the full frame; the view steps preprocess_views -> backbone -> head -> decode_rows of the whole view list, timed per pass (host clock around a device
          synchronise) -> mean time of one step.  Also merge_views_kernel at the shape both entries accept (8 sources x 20 views x 200 rows).
  merge   this checkout: the same view list through the same steps once, then Engine.merge_views_large on its rows; the same entry at
          8 x 20 x 200 rows and on a one-class pool of 262 144 rows (synthetic rows, K = 0 there so that the whole pool is walked).
Times of a merge: `device_ms` is the span of the entry's launches on the stream (the library's profiling events around them), `call_ms`
the host clock around the Engine call, which ends in its one read-back.

    python tools/bench_views_large.py --parent-tree DIR --rounds 3 --repeats 5 [--out profiles/views_large_bench.txt]
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
BIG_HW, TILE, OVERLAP = (8000, 10000), (800, 800), 0.2


def synthetic_rows(torch, n_src, views_per_src, max_in, n_classes, extent, seed):
    """random rows on the device: boxes of 30 ... 80 pixels anywhere in an extent x extent source, scores descending inside a view"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    nv = n_src * views_per_src
    c = torch.rand(nv, max_in, 2, device="cuda", generator=g) * extent
    wh = 30 + 50 * torch.rand(nv, max_in, 2, device="cuda", generator=g)
    boxes = torch.cat([c - wh / 2, c + wh / 2], dim=2).contiguous()
    scores = torch.rand(nv, max_in, device="cuda", generator=g).sort(dim=1, descending=True).values.contiguous()
    classes = torch.randint(0, n_classes, (nv, max_in), device="cuda", generator=g, dtype=torch.int32)
    counts = torch.full((nv,), max_in, device="cuda", dtype=torch.int32)
    table = [{"source": v % n_src, "crop": (0, 0, extent, extent), "flip": False} for v in range(nv)]
    return table, {"boxes": boxes, "scores": scores, "classes": classes, "counts": counts}


def time_merge(torch, eng, fn, kern, repeats):
    """fn() -> merged list; -> device span of the kernel record `kern` and host time of the call, medians over `repeats`"""
    fn()
    dev, call = [], []
    for _ in range(repeats):
        eng.profile_enable(True)
        eng.profile_read()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        call.append((time.perf_counter() - t0) * 1e3)
        dev.append(eng.profile_read()["kernels"][kern]["ms"])
        eng.profile_enable(False)
    return {"device_ms": statistics.median(dev), "call_ms": statistics.median(call), "device_ms_all": dev,
            "rows_out": [int(o["scores"].numel()) for o in out][:4]}


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

    res = {"leg": args.leg, "tree": os.path.abspath(args.tree), "views": len(table), "steps": len(steps),
           "rows": len(table) * eng.default_max_out()}
    both = synthetic_rows(torch, 8, 20, 200, 5, 1000, 1)
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
        res["block_merge_8x20x200"] = time_merge(torch, eng, lambda: eng.merge_views(both[0], both[1], max_out=400), "merge_views_kernel", args.repeats)
    else:
        rows = run_steps()
        res["rows_decoded"] = int(rows["counts"].sum().item())
        res["large_merge_big"] = time_merge(torch, eng, lambda: eng.merge_views_large(table, rows), "merge_large_kernels", args.repeats)
        res["large_merge_8x20x200"] = time_merge(torch, eng, lambda: eng.merge_views_large(both[0], both[1], max_out=400), "merge_large_kernels",
                                                 args.repeats)
        one = synthetic_rows(torch, 1, 1024, 256, 1, 8000, 2)
        res["large_merge_one_class_262144"] = time_merge(torch, eng, lambda: eng.merge_views_large(one[0], one[1], max_out=262144, topk=0),
                                                         "merge_large_kernels", max(2, args.repeats // 2))
    print("BENCH_VIEWS_LARGE_CHILD " + json.dumps(res), flush=True)


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
            line = [l for l in p.stdout.splitlines() if l.startswith("BENCH_VIEWS_LARGE_CHILD ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"{leg} child of round {rnd} failed with {p.returncode}")
            runs[leg].append(json.loads(line[-1][len("BENCH_VIEWS_LARGE_CHILD "):]))
            print(f"round {rnd} {leg} done", file=sys.stderr, flush=True)
    passes = [m for r in runs["steps"] for m in r["steps_ms"]]
    n_steps = runs["steps"][0]["steps"]
    med = lambda key, field: statistics.median(r[key][field] for r in runs["merge" if key.startswith("large") else "steps"])
    out = {"views": runs["steps"][0]["views"], "steps": n_steps, "rows": runs["steps"][0]["rows"], "rows_decoded": runs["merge"][0]["rows_decoded"],
           "parent_steps_ms": {"min": min(passes), "median": statistics.median(passes), "max": max(passes), "passes": len(passes)},
           "parent_mean_step_ms": statistics.median(passes) / n_steps}
    for key in ("large_merge_big", "large_merge_8x20x200", "large_merge_one_class_262144", "block_merge_8x20x200"):
        out[key] = {"device_ms": med(key, "device_ms"), "call_ms": med(key, "call_ms"),
                    "rows_out": runs["merge" if key.startswith("large") else "steps"][0][key]["rows_out"]}
    out["merge_below_one_step"] = out["large_merge_big"]["call_ms"] < out["parent_mean_step_ms"]
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
