"""TFA-style fine-tuning on the K shots: the baseline the reference compares Sylph against (MODEL.TFA.*, FREEZE_CLS_TOWER,
FREEZE_BBOX_TOWER).  configs/COCO-Detection/TFA/FCOS_finetune.yaml and the "-simplified" yamls train only the last classifier layer
(FREEZE_BBOX_BRANCH); the Meta-FCOS-pretrain-tfa-finetune yamls also train the box branch.

Class codes (finetune_class_codes): a record keeps the cls tower's output, so one gradient step is one streaming pass over it per 32
classes (csrc/finetune.hip) -- no backbone, no towers, no autograd graph.  The optimiser acts on 257 N floats and stays in torch.
The box branch (finetune_box_branch, below): bbox_pred / ctrness / iou_overlap and the level scales on a box-sample bank -- the 3x3x256
patches of the frozen bbox tower at the positive locations, cut out once per batch -- one launch per step (csrc/box_finetune.hip).

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


def _single_rank(who: str):
    """every training entry here steps on one rank's gradients: refused by name under a larger world"""
    from . import distributed as D
    if D.get_world_size() > 1:
        raise NotImplementedError(f"{who}: gradients are not reduced across ranks; world size is {D.get_world_size()}")


class MasterSGD:
    """torch.optim.SGD + MultiStepLR over fp32 master tensors: the shell of CodeOptimizer, BranchOptimizer and GeneratorOptimizer, which
    add how kernel outputs become `.grad`.  `_freeze(master, frozen)` saves the master as it stands; after every step its elements
    under the bool mask `frozen` (broadcast against it) get the saved bits back, so neither the gradient nor weight decay nor momentum
    moves them."""

    def _init_sgd(self, masters, *, lr: float, momentum: float, weight_decay: float, lr_steps: Sequence[int], lr_gamma: float):
        self._masters = list(masters)
        self._frozen = []
        self.opt = torch.optim.SGD(self._masters, lr=lr, momentum=momentum, weight_decay=weight_decay)
        self.sched = torch.optim.lr_scheduler.MultiStepLR(self.opt, milestones=sorted(int(s) for s in lr_steps), gamma=lr_gamma)

    @property
    def lr(self) -> float:
        return self.opt.param_groups[0]["lr"]

    def _freeze(self, master: torch.Tensor, frozen: torch.Tensor):
        self._frozen.append((master, master.clone(), frozen.to(master.device)))

    def _sgd_step(self, *grads: torch.Tensor):
        """one gradient per master, in their order: step, schedule, put the frozen elements back"""
        for p, g in zip(self._masters, grads):
            p.grad = g
        self.opt.step()
        self.sched.step()
        for p, p0, frozen in self._frozen:
            p.copy_(torch.where(frozen, p0, p))


class CodeOptimizer(MasterSGD):
    """fp32 master copies of the codes.  `step` takes the gradient SUMS of the step's records and the number of positive locations,
    divides by max(num_pos, 1) (fcos_outputs.py:651, one rank) and steps.  Rows whose `trainable` entry is False keep their bits (TFA's
    USE_PRETRAINED_BASE_CLS_LOGITS keeps the base classes fixed this way)."""

    def __init__(self, cls_conv: torch.Tensor, cls_bias: Optional[torch.Tensor], *, lr: float, momentum: float = 0.9, weight_decay: float = 1e-4,
                 trainable=None, lr_steps: Sequence[int] = (), lr_gamma: float = 0.1):
        n = cls_conv.shape[0]
        if cls_conv.numel() != n * 256:
            raise ValueError(f"finetune_class_codes: 3x3 class codes are not supported: cls_conv must be (N, 256, 1, 1), not {tuple(cls_conv.shape)}")
        self.w = cls_conv.detach().to(torch.float32).reshape(n, 256).clone()
        self.b = cls_bias.detach().to(self.w.device, torch.float32).reshape(-1).clone() if cls_bias is not None else None
        if self.b is not None and self.b.numel() != n:
            raise ValueError(f"finetune_class_codes: {self.b.numel()} biases for {n} classes")
        self._init_sgd([self.w] + ([self.b] if self.b is not None else []), lr=lr, momentum=momentum, weight_decay=weight_decay,
                       lr_steps=lr_steps, lr_gamma=lr_gamma)
        if trainable is not None:
            m = torch.as_tensor(trainable, dtype=torch.bool).reshape(-1)
            if m.numel() != n:
                raise ValueError(f"finetune_class_codes: trainable has {m.numel()} entries for {n} classes")
            if not bool(m.all()):
                self._freeze(self.w, ~m.reshape(n, 1))
                if self.b is not None:
                    self._freeze(self.b, ~m)

    def step(self, grad_w_sum: torch.Tensor, grad_b_sum: Optional[torch.Tensor], num_pos: torch.Tensor):
        norm = num_pos.reshape(()).clamp(min=1).to(torch.float32)
        self._sgd_step(grad_w_sum / norm, *([grad_b_sum / norm] if self.b is not None else []))
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
    _single_rank("finetune_class_codes")
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


# ---- the box branch (the Meta-FCOS-pretrain-tfa-finetune yamls: FREEZE_BBOX_TOWER on, FREEZE_BBOX_BRANCH off) --------------------------
BOX_BRANCH_PARTS = ("bbox_pred", "ctrness", "iou_overlap")


def stack_box_branch(branch: Dict[str, torch.Tensor]):
    """{"bbox_pred.weight|bias", "ctrness.*"[, "iou_overlap.*"], "scales.{l}.scale"} -> (w (Cout, 256, 3, 3), b (Cout,), scales (levels,))"""
    parts = [p for p in BOX_BRANCH_PARTS if f"{p}.weight" in branch]
    if parts[:2] != ["bbox_pred", "ctrness"]:
        raise ValueError(f"box branch: bbox_pred and ctrness are required, got {sorted(branch)}")
    w = torch.cat([branch[f"{p}.weight"].float() for p in parts])
    b = torch.cat([branch[f"{p}.bias"].float().reshape(-1) for p in parts])
    L = 0
    while f"scales.{L}.scale" in branch:
        L += 1
    s = torch.stack([branch[f"scales.{l}.scale"].float().reshape(()) for l in range(L)]) if L else torch.zeros(0)
    return w, b, s


def split_box_branch(w: torch.Tensor, b: torch.Tensor, scales: torch.Tensor) -> Dict[str, torch.Tensor]:
    """the inverse of stack_box_branch (Cout 5: no iou_overlap)"""
    out, n0 = {}, 0
    for p, co in zip(BOX_BRANCH_PARTS, (4, 1, 1)):
        if n0 >= w.shape[0]:
            break
        out[f"{p}.weight"] = w[n0:n0 + co].clone()
        out[f"{p}.bias"] = b[n0:n0 + co].clone()
        n0 += co
    for l in range(scales.numel()):
        out[f"scales.{l}.scale"] = scales[l].reshape(1).clone()
    return out


def box_loss_norms(sums: torch.Tensor, n: int, quality: Sequence[str]):
    """fcos_outputs.py:698-738 on one rank: (the divisor of loss_fcos_loc, num_pos_avg) as 0-d device tensors.  loc is divided by
    max(sum of centerness targets, 1e-6) when "ctrness" weights it, by num_pos_avg = max(n, 1) under ["iou"] alone."""
    npos = torch.tensor(float(max(int(n), 1)), device=sums.device)
    return (sums[3].clamp(min=1e-6) if "ctrness" in quality else npos), npos


class BranchOptimizer(MasterSGD):
    """fp32 masters of the box branch, as CodeOptimizer keeps the codes.  `step` takes box_grad's un-normalised gradients and the two
    divisors.  Parts that receive no gradient -- the quality channel BOX_QUALITY does not name, the scales without USE_SCALE -- keep
    their bits."""

    def __init__(self, w: torch.Tensor, b: torch.Tensor, scales: torch.Tensor, quality: Sequence[str], *, lr: float, momentum: float = 0.9,
                 weight_decay: float = 1e-4, lr_steps: Sequence[int] = (), lr_gamma: float = 0.1, train_scales: bool = True):
        self.w, self.b, self.s = (t.detach().to(torch.float32).clone() for t in (w, b, scales))
        self._init_sgd([self.w, self.b, self.s], lr=lr, momentum=momentum, weight_decay=weight_decay, lr_steps=lr_steps, lr_gamma=lr_gamma)
        cout = self.w.shape[0]
        frozen = torch.zeros(cout, dtype=torch.bool)
        if "ctrness" not in quality:
            frozen[4] = True
        if cout > 5 and "iou" not in quality:
            frozen[5] = True
        if bool(frozen.any()):
            self._freeze(self.w, frozen.reshape(cout, 1, 1, 1))
            self._freeze(self.b, frozen)
        if not train_scales:
            self._freeze(self.s, torch.ones(1, dtype=torch.bool))

    def step(self, grad_w: torch.Tensor, grad_b: torch.Tensor, grad_scales: torch.Tensor, loc_norm: torch.Tensor, num_pos: torch.Tensor):
        div = torch.cat([loc_norm.reshape(1).expand(4), num_pos.reshape(1).expand(self.w.shape[0] - 4)])
        self._sgd_step(grad_w / div.reshape(-1, 1, 1, 1), grad_b / div, grad_scales / loc_norm)


def finetune_box_branch(engine_or_model, samples, branch: Dict[str, torch.Tensor], *, iters: int, lr: float, momentum: float = 0.9,
                        weight_decay: float = 1e-4, lr_steps: Sequence[int] = (), lr_gamma: float = 0.1,
                        samples_per_step: Optional[int] = None, seed: int = 0):
    """Train `branch` (Engine.box_branch()'s dict) on the box-sample bank `samples` (Engine.box_samples, BoxSamples.cat): per step one
    box_grad launch over the bank -- or over the next `samples_per_step` of a stream of seeded permutations -- the gradients divided as
    fcos_outputs.py:698-738 divides the losses, one SGD step.  BOX_QUALITY / IOU_MASK come from cfg.MODEL.FCOS.  Returns (branch, losses):
    the trained dict (not installed: Engine.set_box_branch does that) and the normalised (loc, ctr, iou) losses of every step as one
    (iters, 3) device tensor."""
    _single_rank("finetune_box_branch")
    eng = getattr(engine_or_model, "engine", engine_or_model)
    quality = sorted(eng.fcos_train["box_quality"])
    w, b, s = (t.to(eng.device) for t in stack_box_branch(branch))
    opt = BranchOptimizer(w, b, s, quality, lr=lr, momentum=momentum, weight_decay=weight_decay, lr_steps=lr_steps, lr_gamma=lr_gamma,
                          train_scales=bool(eng.sc.use_scale))
    n = samples.n
    if samples_per_step is None or int(samples_per_step) >= n:
        plan = None
    else:
        plan = step_records(n, int(samples_per_step), int(iters), seed)
    losses = torch.zeros(int(iters), 3, device=eng.device)
    for it in range(int(iters)):
        bank = samples if plan is None else samples.select(torch.tensor(plan[it], device=eng.device))
        out = eng.box_grad(bank, opt.w, opt.b, opt.s)
        loc_norm, npos = box_loss_norms(out["sums"], bank.n, quality)
        losses[it] = out["sums"][:3] / torch.stack([loc_norm, npos, npos])
        opt.step(out["grad_w"], out["grad_b"], out["grad_scales"], loc_norm, npos)
    return {k: v.cpu() for k, v in split_box_branch(opt.w, opt.b, opt.s).items()}, losses
