"""Cost of the MobileNetV2 backbone (bf16, MODEL.MOBILENET True) in a 5-way query step from host images (preprocess + backbone + FPN +
head + decode) on 800x1333 images padded to 800x1344, synthetic weights -- the protocol of tools/bench_resnet_basic.py -- next to the
R-18 step under the same protocol, the two alternating in one process.

Per batch size it prints one JSON line per backbone and repetition: the whole-step time (HIP events, img/s) and the per-kernel times of
the launches the library times itself.  --layers adds the per-block table: each of the 17 InvertedResidual blocks alone, at the map size
it has in the network, once as the three-launch chain (SYLPH_MBV2_FUSED 0) and once as the one-launch kernel (2), through
Engine.mbv2_block.  chain_ms / fused_ms are the SUM OF THE BLOCK'S OWN KERNEL TIMES (HIP events around each launch the library times),
not wall time: the import / export of the parity entry is left out.  With them the algorithmic bytes of the block (input + output map;
the hidden tensors are what the fused kernel keeps on chip) and of the chain (the same plus one write and one read of each hidden
tensor); chain_TBps is chain_GB over chain_ms, so it too is kernel time only.

    python tools/bench_mobilenet.py --batches 192 64 --steps 3 --reps 3 [--layers 16] [--out profiles/mobilenet_bench.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "sylph-few-shot-detection_amd"))

import torch  # noqa: E402


def cfg_for(backbone):
    from sylph_amd.config import get_default_cfg
    cfg = get_default_cfg()
    cg = cfg.MODEL.META_LEARN.CODE_GENERATOR
    cfg.MODEL.META_LEARN.EPISODIC_LEARNING = True
    cg.CONV_L2_NORM = True
    cg.TOWER_LAYERS = [["GN", "ReLU"], ["GN", "ReLU"]]
    cg.CLS_LAYER = ["", "", 1]
    cg.BIAS_LAYER = ["", "", 1]
    if backbone == "MobileNetV2":
        cfg.MODEL.MOBILENET = True
    else:
        cfg.MODEL.RESNETS.DEPTH, cfg.MODEL.RESNETS.RES2_OUT_CHANNELS = 18, 64
    return cfg


class Step:
    def __init__(self, backbone, B):
        from sylph_amd import synthetic as Wt
        from sylph_amd.engine import Engine
        self.backbone, self.B = backbone, B
        self.eng = Engine(cfg_for(backbone), dtype="bf16")
        sd = Wt.mobilenet_backbone_state_dict(0) if backbone == "MobileNetV2" else Wt.backbone_state_dict(0, depth=18)
        sd.update(Wt.head_state_dict(1, num_classes=60))
        self.eng.load_state_dict(sd)
        four = Wt.synthetic_images(4, 800, 1333, seed=3)
        self.imgs = [four[i % 4] for i in range(B)]
        self.codes = Wt.synthetic_codes(5, seed=4, scale=3.0)

    def __call__(self):
        e = self.eng
        e.preprocess(self.imgs)
        e.backbone()
        e.head(self.codes["cls_conv"], self.codes["cls_bias"])
        return e.decode()

    def timed(self, steps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            self()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / steps

    def kernels(self, steps):
        e = self.eng
        e.profile_enable(True)
        e.profile_read()
        for _ in range(steps):
            self()
        torch.cuda.synchronize()
        kern = e.profile_read()["kernels"]
        e.profile_enable(False)
        return {k: {"ms_per_step": v["ms"] / steps, "launches_per_step": v["launches"] / steps} for k, v in kern.items()}


def layer_table(B, iters=3, H=800, W=1344):
    """the 17 blocks alone at their map sizes, B images"""
    from sylph_amd import synthetic as Wt
    from sylph_amd.engine import Engine
    eng = Engine(cfg_for("MobileNetV2"), dtype="bf16")
    eng.profile_enable(True)
    g = torch.Generator().manual_seed(0)
    h, w = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    rows = []
    for fi, (cin, t, cout, stride) in enumerate(Wt.mobilenet_v2_blocks(), start=1):
        hid = cin * t
        ws = [None if t == 1 else torch.randn(hid, cin, 1, 1, generator=g) * (3.0 / cin ** 0.5), torch.randn(hid, 1, 3, 3, generator=g) * 0.4,
              torch.randn(cout, hid, 1, 1, generator=g) * (0.4 / hid ** 0.5)]
        ch = [hid, hid, cout]
        sc = [None if ws[i] is None else torch.ones(ch[i]) for i in range(3)]
        sh = [None if ws[i] is None else torch.full((ch[i],), 0.5) for i in range(3)]
        x = torch.randn(B, cin, h, w, generator=g)
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        ms, launches = {}, {}
        for route, knob in (("chain", "0"), ("fused", "2")):
            os.environ["SYLPH_MBV2_FUSED"] = knob  # read at every pick_mbv2_route
            eng.mbv2_block(x, ws, sc, sh, stride)
            eng.profile_read()
            for _ in range(iters):
                eng.mbv2_block(x, ws, sc, sh, stride)
            torch.cuda.synchronize()
            kern = eng.profile_read()["kernels"]
            ms[route] = sum(v["ms"] for v in kern.values()) / iters  # kernel time only
            launches[route] = {k: v["launches"] // iters for k, v in kern.items()}
        os.environ.pop("SYLPH_MBV2_FUSED")
        pc = eng.mbv2_padded_channels
        io = 2 * B * (h * w * pc(cin) * (2 if stride == 1 and cin == cout else 1) + ho * wo * pc(cout))
        hidden = 2 * B * ((2 * h * w * pc(hid) if t != 1 else 0) + 2 * ho * wo * pc(hid))
        rows.append({"features": fi, "cin": cin, "t": t, "cout": cout, "stride": stride, "map": [h, w], "batch": B, "chain_ms": ms["chain"],
                     "fused_ms": ms["fused"], "launches": launches, "block_GB": io / 1e9, "chain_GB": (io + hidden) / 1e9,
                     "chain_TBps": (io + hidden) / (ms["chain"] * 1e-3) / 1e12})
        print(json.dumps(rows[-1]), flush=True)
        h, w = ho, wo
        del x
        torch.cuda.empty_cache()
    eng.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[192, 64])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3, help="alternations MobileNetV2 / R-18 per batch size")
    ap.add_argument("--layers", type=int, default=0, help="batch size of the per-block table (0: no table)")
    ap.add_argument("--out", default=None, help="also write every line to this file")
    args = ap.parse_args()
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    for B in args.batches:
        steps = {name: Step(name, B) for name in ("MobileNetV2", "R-18")}
        for s in steps.values():
            for _ in range(args.warmup):
                s()
        for rep in range(args.reps):
            for name, s in steps.items():
                ms = s.timed(args.steps)
                emit({"backbone": name, "batch": B, "rep": rep, "step_ms": ms, "img_per_s": B / (ms * 1e-3)})
        for name, s in steps.items():
            emit({"backbone": name, "batch": B, "kernels": s.kernels(args.steps)})
            s.eng.close()
        del steps
        torch.cuda.empty_cache()
    if args.layers:
        for row in layer_table(args.layers):
            lines.append(json.dumps(row))
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"# bf16, 800x1333 images padded to 800x1344, 5 classes, preprocess + backbone + FPN + head + decode, {args.warmup} warm-up + "
                    f"{args.steps} timed steps (HIP events) per repetition, MobileNetV2 and R-18 alternating, synthetic weights\n")
            if args.layers:
                f.write("# per-block rows: chain_ms / fused_ms / chain_TBps count the block's own kernels only (HIP events per launch), not wall time\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
