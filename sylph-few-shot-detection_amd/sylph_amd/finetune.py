"""TFA-style fine-tuning of class codes on query records: the baseline the reference compares Sylph against
(configs/COCO-Detection/TFA/FCOS_finetune.yaml: FREEZE_CLS_TOWER, FREEZE_BBOX_TOWER, MODEL.TFA.*), which trains only the last classifier
layer on the K shots.  A record keeps the cls tower's output, so one gradient step is one streaming pass over it per 32 classes
(csrc/finetune.hip) -- no backbone, no towers, no autograd graph.  The optimiser acts on 257 N floats and stays in torch.

    codes, losses = finetune_class_codes(engine, records, annotations, class_codes, iters=200, lr=0.02)
    model(record_inputs, class_code=codes, run_type="meta_learn_test_instance")

`class_codes` is either what "meta_learn_test_support" + "meta_learn_normalize_code" returned, or a base detector's own cls_logits rows
(`MetaOneStageDetector._pretrained_class_codes`)."""
import math
from typing import Dict, List, Optional, Sequence

import torch


def prior_bias(prior_prob: float) -> float:
    """fcos.py:432-433: the bias a classifier starts from, -log((1 - pi) / pi)"""
    return -math.log((1.0 - prior_prob) / prior_prob)


def step_records(n_records: int, records_per_step: Optional[int], iters: int, seed: int) -> List[List[int]]:
    """Which records each step reads: all of them, or the next `records_per_step` of a stream of seeded permutations (every record is
    read once before any is read twice)."""
    if n_records <= 0:
        raise ValueError("finetune_class_codes: no records")
    r = n_records if records_per_step is None else int(records_per_step)
    if r <= 0 or r > n_records:
        raise ValueError(f"finetune_class_codes: records_per_step {records_per_step} with {n_records} records")
    if r == n_records:
        return [list(range(n_records))] * iters
    g = torch.Generator().manual_seed(int(seed))
    stream: List[int] = []
    while len(stream) < r * iters:
        stream += torch.randperm(n_records, generator=g).tolist()
    return [stream[i * r:(i + 1) * r] for i in range(iters)]


class CodeOptimizer:
    """fp32 master copies of the codes under torch.optim.SGD + MultiStepLR.  `step` takes the gradient SUMS of the step's records and the
    number of positive locations, divides by max(num_pos, 1) (fcos_outputs.py:651, one rank) and steps.  Rows whose `trainable` entry is
    False keep their bits: neither the gradient nor weight decay nor momentum moves them (TFA's USE_PRETRAINED_BASE_CLS_LOGITS keeps
    the base classes fixed this way)."""

    def __init__(self, cls_conv: torch.Tensor, cls_bias: Optional[torch.Tensor], *, lr: float, momentum: float = 0.9, weight_decay: float = 1e-4,
                 trainable=None, lr_steps: Sequence[int] = (), lr_gamma: float = 0.1):
        n = cls_conv.shape[0]
        if cls_conv.numel() != n * 256:
            raise ValueError(f"finetune_class_codes: 3x3 class codes are not supported: cls_conv must be (N, 256, 1, 1), not {tuple(cls_conv.shape)}")
        self.w = cls_conv.detach().to(torch.float32).reshape(n, 256).clone()
        self.b = cls_bias.detach().to(self.w.device, torch.float32).reshape(-1).clone() if cls_bias is not None else None
        if self.b is not None and self.b.numel() != n:
            raise ValueError(f"finetune_class_codes: {self.b.numel()} biases for {n} classes")
        self.frozen = None
        if trainable is not None:
            m = torch.as_tensor(trainable, dtype=torch.bool).reshape(-1)
            if m.numel() != n:
                raise ValueError(f"finetune_class_codes: trainable has {m.numel()} entries for {n} classes")
            if not bool(m.all()):
                self.frozen = (~m).to(self.w.device)
                self.w0 = self.w.clone()
                self.b0 = self.b.clone() if self.b is not None else None
        params = [self.w] + ([self.b] if self.b is not None else [])
        self.opt = torch.optim.SGD(params, lr=lr, momentum=momentum, weight_decay=weight_decay)
        self.sched = torch.optim.lr_scheduler.MultiStepLR(self.opt, milestones=sorted(int(s) for s in lr_steps), gamma=lr_gamma)

    @property
    def lr(self) -> float:
        return self.opt.param_groups[0]["lr"]

    def step(self, grad_w_sum: torch.Tensor, grad_b_sum: Optional[torch.Tensor], num_pos: torch.Tensor):
        norm = num_pos.reshape(()).clamp(min=1).to(torch.float32)
        self.w.grad = grad_w_sum / norm
        if self.b is not None:
            self.b.grad = grad_b_sum / norm
        self.opt.step()
        self.sched.step()
        if self.frozen is not None:
            self.w[self.frozen] = self.w0[self.frozen]
            if self.b is not None:
                self.b[self.frozen] = self.b0[self.frozen]
        return norm


def _check_annotations(annotations, records, n_classes: int):
    if len(annotations) != len(records):
        raise ValueError(f"finetune_class_codes: {len(annotations)} annotations for {len(records)} records")
    out = []
    for i, a in enumerate(annotations):
        bx = torch.as_tensor(a["boxes"], dtype=torch.float32).reshape(-1, 4).cpu()
        cl = torch.as_tensor(a["classes"]).reshape(-1).cpu().long()
        im = torch.as_tensor(a["image_index"]).reshape(-1).cpu().long()
        if cl.numel() and (int(cl.max()) >= n_classes or int(cl.min()) < 0):
            raise ValueError(f"finetune_class_codes: record {i} has a label >= N or a negative one (classes {int(cl.min())} .. {int(cl.max())}, "
                             f"{n_classes} class codes)")
        out.append((bx, cl, im))
    return out


def finetune_class_codes(engine_or_model, records, annotations, class_codes: Dict[str, torch.Tensor], *, iters: int, lr: float,
                         momentum: float = 0.9, weight_decay: float = 1e-4, records_per_step: Optional[int] = None, trainable=None,
                         lr_steps: Sequence[int] = (), lr_gamma: float = 0.1, seed: int = 0):
    """Refine `class_codes` ({"cls_conv": (N, 256, 1, 1), "cls_bias": (N,) or absent}) on `records` (QueryRecords of the support images)
    with `annotations` (per record {"boxes": (n, 4) in network-input pixels, "classes": (n,), "image_index": (n,) sorted}).  Per step:
    load_record + cls_grad for each record of the step, gradients summed, divided by max(sum num_pos, 1), one SGD step.  Focal alpha /
    gamma and the target assignment come from cfg.MODEL.FCOS.  Returns (codes, losses): the dict "meta_learn_test_instance" takes, and
    the normalised loss of every step as one device tensor (read it back once, at the end)."""
    from . import distributed as D
    if D.get_world_size() > 1:
        raise NotImplementedError(f"finetune_class_codes: gradients are not reduced across ranks; world size is {D.get_world_size()}")
    eng = getattr(engine_or_model, "engine", engine_or_model)
    w_in, b_in = class_codes["cls_conv"], class_codes.get("cls_bias")
    opt = CodeOptimizer(w_in.to(eng.device), b_in, lr=lr, momentum=momentum, weight_decay=weight_decay, trainable=trainable, lr_steps=lr_steps,
                        lr_gamma=lr_gamma)
    n = opt.w.shape[0]
    ann = _check_annotations(annotations, records, n)
    plan = step_records(len(records), records_per_step, int(iters), seed)
    targets = []
    for rec, (bx, cl, im) in zip(records, ann):  # once per record
        eng.load_record(rec)
        targets.append(eng.fcos_targets(bx, cl, im))
    losses = torch.zeros(int(iters), device=eng.device)
    for it, recs in enumerate(plan):
        gw = torch.zeros_like(opt.w)
        gb = torch.zeros_like(opt.b) if opt.b is not None else None
        loss = torch.zeros(1, device=eng.device)
        npos = torch.zeros(1, device=eng.device, dtype=torch.int32)
        for r in recs:
            eng.load_record(records[r])
            l1, gw1, gb1 = eng.cls_grad(targets[r][0], opt.w, opt.b, check_labels=False)
            gw += gw1
            if gb is not None:
                gb += gb1
            loss += l1
            npos += targets[r][1]
        norm = opt.step(gw, gb, npos)
        losses[it] = (loss / norm)[0]
    out = {"cls_conv": opt.w.reshape(n, 256, 1, 1).to(w_in.dtype)}
    if opt.b is not None:
        out["cls_bias"] = opt.b.reshape(b_in.shape).to(b_in.dtype)
    return out, losses
