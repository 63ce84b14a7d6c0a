"""Cost of fine-tuning the box branch on a box-sample bank (sylph_box_samples / sylph_box_grad, sylph_amd.finetune.finetune_box_branch).
bf16, R-50-FPN synthetic weights, 20-way 10-shot: 200 support images of 800x1333 (padded to 800x1344), one box each, in passes of
--batch images.  Per round (--rounds, default 3), every leg once, alternating; per leg the median, min and max (wall ms, synchronised):

  towers           Engine.towers() on the batch (backbone excluded): the pass the samples ride on
  targets          Engine.fcos_targets on that batch
  samples          Engine.box_samples on that batch (its four launches and the read-back of the count)
  grad_step        Engine.box_grad over the WHOLE bank + BranchOptimizer.step: one SGD step of finetune_box_branch
  autograd_step    the yardstick: the same formulas in torch (fp32 on the same device tensors: bf16 patches, bf16-rounded weights), loss.backward()
                   and the same optimiser step.  Not the kernel: the restatement is what a user would write without it.

and the bank's sample count and bytes.  One JSON line.
    python tools/bench_box_finetune.py --batch 100
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
import torch.nn.functional as F  # noqa: E402

from bench_records import build_model, wall  # noqa: E402


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "rounds": len(v)}


def autograd_losses(x, tau, lv, w, b, s, quality):
    """fcos_outputs.py:675-741 + iou_loss.py:26-65 on one rank, normalised; x (n, 2304) fp32, w (Cout, 256, 3, 3)"""
    wq = w.to(torch.bfloat16).float().permute(0, 2, 3, 1).reshape(w.shape[0], -1)
    z = x @ wq.t() + b
    p = torch.relu(s[lv][:, None] * z[:, :4])
    ta = (tau[:, 0] + tau[:, 2]) * (tau[:, 1] + tau[:, 3])
    pa = (p[:, 0] + p[:, 2]) * (p[:, 1] + p[:, 3])
    wi = torch.min(p[:, 0], tau[:, 0]) + torch.min(p[:, 2], tau[:, 2])
    hi = torch.min(p[:, 3], tau[:, 3]) + torch.min(p[:, 1], tau[:, 1])
    ac = (torch.max(p[:, 0], tau[:, 0]) + torch.max(p[:, 2], tau[:, 2])) * (torch.max(p[:, 3], tau[:, 3]) + torch.max(p[:, 1], tau[:, 1]))
    ai = wi * hi
    au = ta + pa - ai
    iou = (ai + 1.0) / (au + 1.0)
    giou = iou - (ac - au) / ac
    lr, tb = tau[:, [0, 2]], tau[:, [1, 3]]
    ctr_t = torch.sqrt((lr.min(-1)[0] / lr.max(-1)[0]) * (tb.min(-1)[0] / tb.max(-1)[0]))
    npos = max(float(x.shape[0]), 1.0)
    total = 0
    if "ctrness" in quality:
        total = total + ((1 - giou) * ctr_t).sum() / ctr_t.sum().clamp(min=1e-6) + F.binary_cross_entropy_with_logits(z[:, 4], ctr_t, reduction="sum") / npos
    else:
        total = total + (1 - giou).sum() / npos
    if "iou" in quality:
        total = total + F.binary_cross_entropy_with_logits(z[:, 5], iou.detach(), reduction="sum") / npos
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ways", type=int, default=20)
    ap.add_argument("--shots", type=int, default=10)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_box_finetune.py needs a GPU")
    from sylph_amd import synthetic as Wt
    from sylph_amd.engine import BoxSamples
    from sylph_amd.finetune import BranchOptimizer, box_loss_norms, stack_box_branch
    model = build_model()
    eng = model.engine
    quality = sorted(eng.fcos_train["box_quality"])
    n_img = args.ways * args.shots
    base = [im.cuda() for im in Wt.synthetic_images(4, 800, 1333, seed=9)]
    boxes = Wt.synthetic_boxes(n_img, 800, 1333, seed=11)
    ms = {k: [] for k in ("towers", "targets", "samples", "grad_step", "autograd_step")}
    banks = []
    for it in range(1 + args.rounds):  # one warm-up round
        banks = []
        for i in range(0, n_img, args.batch):
            idx = list(range(i, min(n_img, i + args.batch)))
            model._run_backbone([{"image": base[j % 4], "height": 800, "width": 1333} for j in idx])
            ann = (boxes[idx], torch.tensor([j % args.ways for j in idx]), torch.arange(len(idx)))
            t = {"towers": wall(eng.towers), "targets": wall(lambda: eng.fcos_targets(*ann))}
            t["samples"] = wall(lambda: banks.append(eng.box_samples(*ann)))
            if it and i == 0:
                for k, v in t.items():
                    ms[k].append(v)
        bank = BoxSamples.cat(banks)
        w, b, s = (t.cuda() for t in stack_box_branch(eng.box_branch()))

        def grad_step(opt):
            out = eng.box_grad(bank, opt.w, opt.b, opt.s)
            loc_norm, npos = box_loss_norms(out["sums"], bank.n, quality)
            opt.step(out["grad_w"], out["grad_b"], out["grad_scales"], loc_norm, npos)

        x32, lv = bank.patches.reshape(bank.n, -1).float(), bank.info[:, 1].long()

        def autograd_step(opt):
            ps = [opt.w.requires_grad_(True), opt.b.requires_grad_(True), opt.s.requires_grad_(True)]
            gw, gb, gs = torch.autograd.grad(autograd_losses(x32, bank.targets, lv, *ps, quality), ps)
            for p in ps:
                p.requires_grad_(False)
            opt.w.grad, opt.b.grad, opt.s.grad = gw, gb, gs
            opt.opt.step()
            opt.sched.step()

        for name, fn in (("grad_step", grad_step), ("autograd_step", autograd_step)):
            opt = BranchOptimizer(w, b, s, quality, lr=5e-4)
            fn(opt)  # (the first call allocates)
            t = wall(lambda: [fn(opt) for _ in range(20)]) / 20
            if it:
                ms[name].append(t)
    res = {"ways": args.ways, "shots": args.shots, "images": n_img, "images_per_pass": args.batch, "box_quality": quality,
           "bank_samples": bank.n, "bank_bytes": bank.nbytes, "ms": {k: summary(v) for k, v in ms.items()}}
    m = res["ms"]
    res["samples_over_towers"] = m["samples"]["median"] / m["towers"]["median"]
    res["grad_step_over_autograd_step"] = m["grad_step"]["median"] / m["autograd_step"]["median"]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
