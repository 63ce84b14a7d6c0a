"""Cost of one meta-training step of the code generator (sylph_codegen_train_forward / sylph_codegen_train_backward).
bf16, synthetic generator weights (two ["GN", "ReLU"] tower layers, bias head, post GroupNorm, L2 norm), a --ways x --shots episode
(default 20 x 5 = 100 shots) drawn from a bank of synthetic ROI rows.  Per round (--rounds, default 3), every leg once, alternating; per
leg the median, min and max (wall ms, synchronised, mean of 20 calls):

  generator_step   Engine.codegen_train_forward + codegen_train_backward: what the kernels do per step
  autograd_step    the yardstick: the same formulas under torch autograd on the same device -- fp32 torch convs on the bf16-rounded
                   weights and the same bank rows, loss = sum(codes * G), torch.autograd.grad to every parameter.  Not the kernel: the
                   restatement is what a user would write without it.

The step's own cls_grad pass over a 100-image record is 0.59 ms at N = 20 (profiles/finetune_bench.txt); it is not timed again here.
One JSON line.
    python tools/bench_codegen_train.py
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
import torch.nn.functional as F  # noqa: E402

P = "code_generator.code_generator_head"


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "rounds": len(v)}


def autograd_codes(x0, p, seg_len, depth, prior):
    """code_generator.py:924-1002, training branch, fp32: x0 (M, 256, 7, 7)"""
    q = lambda w: w + (w.detach().to(torch.bfloat16).float() - w.detach())
    x = x0
    for i in range(depth):
        y = F.conv2d(x, q(p[f"{P}.support_set_shared_tower.{3 * i}.weight"]), p[f"{P}.support_set_shared_tower.{3 * i}.bias"], padding=1)
        x = F.relu(F.group_norm(y, 32, p[f"{P}.support_set_shared_tower.{3 * i + 1}.weight"], p[f"{P}.support_set_shared_tower.{3 * i + 1}.bias"], eps=1e-5))
    c = F.conv2d(x, q(p[f"{P}.support_set_cls_conv.0.weight"]), p[f"{P}.support_set_cls_conv.0.bias"], padding=1).mean(dim=(2, 3))
    rb = F.conv2d(x, q(p[f"{P}.support_set_cls_bias.0.weight"]), p[f"{P}.support_set_cls_bias.0.bias"], padding=1).mean(dim=(2, 3)).reshape(-1)
    n = len(seg_len)
    code = c.reshape(n, seg_len[0], 256).mean(1)
    bias = rb.reshape(n, seg_len[0]).mean(1)
    code = F.normalize(F.group_norm(code, 32, p[f"{P}.post_norm.weight"], p[f"{P}.post_norm.bias"], eps=1e-5), p=2, dim=1) * p[f"{P}.conv_scale.scale"]
    return torch.cat([code, (bias * p[f"{P}.bias_scale.scale"] + prior)[:, None]], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ways", type=int, default=20)
    ap.add_argument("--shots", type=int, default=5)
    ap.add_argument("--bank", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_codegen_train.py needs a GPU")
    import math
    from sylph_amd import synthetic as Wt
    from sylph_amd.config import get_default_cfg
    from sylph_amd.engine import Engine
    cfg = get_default_cfg()
    cfg.MODEL.META_LEARN.EPISODIC_LEARNING = True
    cg = cfg.MODEL.META_LEARN.CODE_GENERATOR
    cg.CONV_L2_NORM = True
    cg.TOWER_LAYERS = [["GN", "ReLU"], ["GN", "ReLU"]]
    cg.CLS_LAYER = ["", "", 1]
    cg.BIAS_LAYER = ["", "", 1]
    eng = Engine(cfg, dtype="bf16")
    sd = Wt.codegen_state_dict(seed=2)
    eng.load_state_dict(sd)
    lay = eng.codegen_params()
    flat = eng.code_generator().cuda()
    M = args.ways * args.shots
    g = torch.Generator().manual_seed(5)
    rows = (torch.rand(args.bank, 49, 256, generator=g) * 2.0).to(torch.bfloat16).cuda()
    idx = torch.randperm(args.bank, generator=g)[:M].tolist()
    seg_len = [args.shots] * args.ways
    G = torch.randn(args.ways, 257, generator=g).cuda()
    x0 = rows[torch.tensor(idx, device="cuda")].float().reshape(M, 7, 7, 256).permute(0, 3, 1, 2).contiguous()
    params = {k: flat[o:o + n].reshape(Engine.codegen_param_shape(k, n)).clone().requires_grad_(True) for k, o, n in lay}
    prior = -math.log((1 - 0.01) / 0.01)

    def generator_step():
        eng.codegen_train_forward(flat, rows, idx, seg_len)
        return eng.codegen_train_backward(G)

    def autograd_step():
        codes = autograd_codes(x0, params, seg_len, 2, prior)
        return torch.autograd.grad((codes * G).sum(), list(params.values()))

    ms = {"generator_step": [], "autograd_step": []}
    for it in range(1 + args.rounds):  # one warm-up round
        for name, fn in (("generator_step", generator_step), ("autograd_step", autograd_step)):
            fn()
            t = wall(lambda: [fn() for _ in range(20)]) / 20
            if it:
                ms[name].append(t)
    got = generator_step()
    want = torch.cat([t.reshape(-1) for t in autograd_step()])
    shp = eng.codegen_train_shape(M, args.ways)
    res = {"ways": args.ways, "shots": args.shots, "rows": M * 49, "units": shp["units"], "passes": shp["passes"],
           "flops_per_step": 2.0 * M * 49 * 2304 * 256 * (2 + 2 + 1) + 6.0 * M * 2304 * 257,
           "grad_cosine_to_autograd": float(F.cosine_similarity(got, want, dim=0)), "ms": {k: summary(v) for k, v in ms.items()}}
    res["generator_step_over_autograd_step"] = res["ms"]["generator_step"]["median"] / res["ms"]["autograd_step"]["median"]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
