"""Cost of running a detector on several VIEWS of the same photograph and merging the results: bf16, R-50-FPN, 5-way, synthetic weights.

Two cases:
  tta    16 sources of 1200 x 1600, scales (600, 800, 1000) with flip: 6 views per source
  tiles  8 sources of 3000 x 4000, 2 x 3 tiles with 20 % overlap plus the full frame (MIN_SIZE_TEST 800 / MAX_SIZE_TEST 1333 per view)
Two legs, each one whole pass from pinned host sources to merged detections on the host side of the API:
  views      model(batch with "views"): sources uploaded once, views cut on the device (sylph_preprocess_views), per-view decode into one
             row buffer, one merge launch (sylph_merge_views), one read-back
  yardstick  what a user can do without those two entries: views cut, resized and flipped on the host (Pillow), one preprocess_u8 step per
             group (the same step grouping), detections copied back, merged on the CPU (a vectorised numpy restatement of
             tests/views_ref.py merge_ref).  --parent-tree DIR runs this leg from another checkout with a build of its own (it uses only
             Engine.preprocess_u8 / backbone / head / decode).
The driver starts one child process per leg and round, alternating the legs --rounds times (>= 3); a child warms up, then times
--repeats passes per case.  Per (case, leg): min, median, max over all passes; the yardstick's max - min is the spread a claim is judged
against.  The views child also reports the merge launch and the preprocess launch on their own (sylph_profile_read_kernels).

    python tools/bench_views.py --rounds 3 --repeats 3 [--parent-tree DIR] [--out profiles/views_bench.txt]
"""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

CASES = {"tta": {"n": 16, "hw": (1200, 1600)}, "tiles": {"n": 8, "hw": (3000, 4000)}}


def load_views_module():
    """sylph_amd/views.py of THIS checkout, by path: host-only, and absent from a parent tree"""
    spec = importlib.util.spec_from_file_location("bench_views_planners", os.path.join(ROOT, "sylph-few-shot-detection_amd", "sylph_amd", "views.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def case_views(V, case):
    h, w = CASES[case]["hw"]
    if case == "tta":
        return V.tta_views(h, w, (600, 800, 1000), 4000, True)
    th, tw = int(h / 1.8 + 0.999), int(w / 2.6 + 0.999)  # 2 rows x 3 columns at 20 % overlap
    return V.tile_views(h, w, (th, tw), 0.2, 800, 1333)


def host_merge(np, table, boxes, scores, classes, n_src, thr, K):
    """merge_ref (tests/views_ref.py), vectorised per kept box: float32, the same order and rules"""
    F = np.float32
    out = []
    for s in range(n_src):
        bs, ss, cs = [], [], []
        for v, t in enumerate(table):
            if t["source"] != s or len(scores[v]) == 0:
                continue
            b = boxes[v].astype(F).copy()
            if t["flip"]:
                cw = F(t["crop"][2])
                b[:, 0], b[:, 2] = cw - boxes[v][:, 2], cw - boxes[v][:, 0]
            b[:, 0::2] += F(t["crop"][0])
            b[:, 1::2] += F(t["crop"][1])
            bs.append(b); ss.append(scores[v]); cs.append(classes[v])
        if not bs:
            out.append((np.zeros((0, 4), F), np.zeros(0, F), np.zeros(0, np.int64)))
            continue
        b, sc, cl = np.concatenate(bs), np.concatenate(ss), np.concatenate(cs)
        order = np.argsort(-sc.astype(np.float64), kind="stable")
        b, sc, cl = b[order], sc[order], cl[order]
        area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        alive = np.ones(len(sc), dtype=bool)
        kept = []
        for i in range(len(sc)):
            if not alive[i]:
                continue
            kept.append(i)
            if thr > 0:
                r = np.nonzero(alive[i + 1:] & (cl[i + 1:] == cl[i]))[0] + i + 1
                if r.size:
                    w = np.maximum(F(0), np.minimum(b[i, 2], b[r, 2]) - np.maximum(b[i, 0], b[r, 0]))
                    h = np.maximum(F(0), np.minimum(b[i, 3], b[r, 3]) - np.maximum(b[i, 1], b[r, 1]))
                    inter = w * h
                    with np.errstate(divide="ignore", invalid="ignore"):
                        alive[r[inter / (area[i] + area[r] - inter) > F(thr)]] = False
        kept = np.asarray(kept, dtype=np.int64)
        if K > 0 and len(kept) > K:
            kept = kept[sc[kept] >= sc[kept[K - 1]]]
        out.append((b[kept], sc[kept], cl[kept]))
    return out


def child(args):
    sys.path.insert(0, args.tree)
    sys.path.insert(0, os.path.join(args.tree, "sylph-few-shot-detection_amd"))
    import numpy as np
    import torch
    from sylph_amd import synthetic as Wt
    from sylph_amd.runner import MetaFCOSRunner, create_cfg
    V = load_views_module()
    r = MetaFCOSRunner()
    cfg = create_cfg(r.get_default_cfg(), "sylph://COCO-Detection/Meta-FCOS/Meta-FCOS-finetune.yaml")
    model = r.build_model(cfg, dtype="bf16")
    model.load_state_dict(Wt.synthetic_state_dict(0, depth=50))
    model.eval()
    eng = model.engine
    codes = {k: v.cuda() for k, v in Wt.synthetic_codes(5, seed=100, scale=3.0).items()}
    thr, K = float(cfg.MODEL.FCOS.NMS_TH), int(cfg.MODEL.FCOS.POST_NMS_TOPK_TEST)
    res = {"leg": args.leg, "tree": os.path.abspath(args.tree), "cases": {}}
    for case in args.cases:
        n, (h, w) = CASES[case]["n"], CASES[case]["hw"]
        g = torch.Generator().manual_seed(7)
        four = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).pin_memory() for _ in range(4)]
        srcs = [four[i % 4] for i in range(n)]
        views = case_views(V, case)

        if args.leg == "views":
            batch = [{"image_u8": s, "resize_hw": (800, 1333), "views": views} for s in srcs]

            def one_pass():
                out = model(batch, class_code=codes, run_type="meta_learn_test_instance")
                return sum(len(o["instances"]) for o in out)
        else:
            from PIL import Image, ImageOps
            table = [dict(v, source=i) for i in range(n) for v in views]
            steps = V.plan_view_steps(table, V.DEFAULT_MAX_BATCH)
            table = [table[i] for st in steps for i in st]
            src_np = [s.numpy() for s in srcs]

            def one_pass():
                boxes, scores, classes = [], [], []
                row0 = 0
                for st in steps:
                    vs = table[row0:row0 + len(st)]
                    imgs = []
                    for v in vs:
                        x0, y0, cw, ch = v["crop"]
                        im = Image.fromarray(src_np[v["source"]]).crop((x0, y0, x0 + cw, y0 + ch)).resize((v["size"][1], v["size"][0]), Image.BILINEAR)
                        if v["flip"]:
                            im = ImageOps.mirror(im)
                        imgs.append(torch.from_numpy(np.asarray(im).copy()).pin_memory())
                    eng.preprocess_u8(imgs, [v["size"] for v in vs])
                    eng.backbone()
                    eng.head(codes["cls_conv"], codes["cls_bias"])
                    for d in eng.decode([(v["crop"][3], v["crop"][2]) for v in vs]):
                        boxes.append(d["pred_boxes"].cpu().numpy()); scores.append(d["scores"].cpu().numpy()); classes.append(d["pred_classes"].cpu().numpy())
                    row0 += len(st)
                return sum(len(m[1]) for m in host_merge(np, table, boxes, scores, classes, n, thr, K))

        for _ in range(args.warmup):
            dets = one_pass()
        ms = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dets = one_pass()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        entry = {"sources": n, "views": n * len(views), "detections": dets, "ms": ms}
        if args.leg == "views":
            eng.profile_enable(True)
            eng.profile_read()
            one_pass()
            torch.cuda.synchronize()
            kern = eng.profile_read()["kernels"]
            eng.profile_enable(False)
            entry["kernels"] = {k: {"ms": kern[k]["ms"], "launches": kern[k].get("launches")} for k in ("view_preprocess_kernel", "merge_views_kernel") if k in kern}
        res["cases"][case] = entry
    print("BENCH_VIEWS_CHILD " + json.dumps(res), flush=True)


def driver(args):
    if args.rounds < 3:
        raise SystemExit("--rounds must be at least 3")
    legs = [("views", ROOT), ("yardstick", args.parent_tree or ROOT)]
    ms = {(c, leg): [] for c in args.cases for leg, _ in legs}
    extra = {}
    for rnd in range(args.rounds):
        for leg, tree in legs:  # alternating: every leg once per round, each in a fresh process
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--tree", tree, "--repeats", str(args.repeats), "--warmup", str(args.warmup),
                   "--cases"] + list(args.cases)
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout)
            line = [l for l in p.stdout.splitlines() if l.startswith("BENCH_VIEWS_CHILD ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"{leg} child of round {rnd} failed with {p.returncode}")
            r = json.loads(line[-1][len("BENCH_VIEWS_CHILD "):])
            for c, e in r["cases"].items():
                ms[(c, leg)] += e["ms"]
                extra[(c, leg)] = {k: e[k] for k in ("sources", "views", "detections", "kernels") if k in e}
            print(f"round {rnd} {leg}: " + ", ".join(f"{c} {min(e['ms']):.1f} ms" for c, e in r["cases"].items()), file=sys.stderr, flush=True)
    lines = []
    for c in args.cases:
        row = {"case": c, "yardstick_tree": "parent" if args.parent_tree else "this checkout (old entries only)"}
        for leg, _ in legs:
            v = ms[(c, leg)]
            row[leg] = dict(extra[(c, leg)], min_ms=min(v), median_ms=statistics.median(v), max_ms=max(v), passes=len(v))
        y, n = row["yardstick"], row["views"]
        row["yardstick_spread_ms"] = y["max_ms"] - y["min_ms"]
        row["yardstick_over_views_median"] = y["median_ms"] / n["median_ms"]
        row["views_win_beyond_spread"] = (y["median_ms"] - n["median_ms"]) > row["yardstick_spread_ms"]
        lines.append(json.dumps(row))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["views", "yardstick"], default=None, help="child mode: time one leg in this process")
    ap.add_argument("--tree", default=ROOT, help="child mode: the checkout whose sylph_amd package and library run the leg")
    ap.add_argument("--parent-tree", default=None, help="driver: a checkout of the parent commit, built, for the yardstick leg")
    ap.add_argument("--cases", nargs="+", default=["tta", "tiles"], choices=sorted(CASES))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--child-timeout", type=int, default=600)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.leg:
        child(args)
    else:
        driver(args)


if __name__ == "__main__":
    main()
