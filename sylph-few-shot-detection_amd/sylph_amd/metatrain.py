"""Meta-training of the code generator on a frozen detector: the paper's second stage, the recipes
configs/LVISv1-Detection/Meta-FCOS/Meta-FCOS-finetune-{once,2,sylph-fa}.yaml and configs/COCO-Detection/Meta-FCOS/Meta-FCOS-finetune-lvis.yaml
(BACKBONE.FREEZE, FREEZE_CLS_TOWER and FREEZE_BBOX_BRANCH on, CODE_GENERATOR.FREEZE off).

With a frozen backbone the 7x7x256 ROI maps of the support instances are constants: a RoiBank keeps them (Engine.roi_rows).  With frozen
towers the query side of an episode is a QueryRecord.  One step draws an episode from the bank, runs the generator's training-mode
forward (csrc/codegen_train.hip), asks cls_grad for d loss / d (code, bias) over the step's records, runs the backward and steps torch
SGD on the flat parameter vector -- no backbone, no towers, no autograd graph.

    bank = build_roi_bank(model, support_loader)
    state, losses = train_code_generator(model, bank, records, annotations, iters=1000, classes_per_step=20, shots=5, records_per_step=2)
    model.set_code_generator(state)
"""
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .finetune import MasterSGD, _single_rank, step_records


def _ints(v) -> List[int]:
    return [int(x) for x in (v.tolist() if hasattr(v, "tolist") else v)]


class RoiBank:
    """rows (n, 49, 256) bf16 on `device`, position-major ROI maps (Engine.roi_rows), + the class id of each row (host list).  The rows
    depend on the backbone alone: they survive every generator update."""

    def __init__(self, device=None):
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        self.rows = torch.empty(0, 49, 256, dtype=torch.bfloat16, device=self.device)
        self.class_ids: List[int] = []
        self._parts: List[torch.Tensor] = []

    def __len__(self) -> int:
        return len(self.class_ids)

    @property
    def nbytes(self) -> int:
        return len(self) * 49 * 256 * 2

    def append(self, rows: torch.Tensor, class_ids: Sequence[int]):
        if rows.dim() != 3 or tuple(rows.shape[1:]) != (49, 256) or rows.dtype != torch.bfloat16:
            raise ValueError(f"ROI bank: rows of shape {tuple(rows.shape)} {rows.dtype}; a bank row is (49, 256) bf16")
        cls = _ints(class_ids)
        if len(cls) != rows.shape[0]:
            raise ValueError(f"ROI bank: {rows.shape[0]} rows with {len(cls)} class ids")
        self._parts.append(rows.detach().to(self.device).clone())
        self.class_ids += cls
        return self

    def tensor(self) -> torch.Tensor:
        if self._parts:
            self.rows = torch.cat([self.rows] + self._parts).contiguous()
            self._parts = []
        return self.rows

    @staticmethod
    def cat(banks: Sequence["RoiBank"]) -> "RoiBank":
        if not banks:
            raise ValueError("ROI bank: nothing to concatenate")
        out = RoiBank(banks[0].device)
        for b in banks:
            if len(b):
                out.append(b.tensor(), b.class_ids)
        out.tensor()
        return out

    def classes(self) -> List[int]:
        return sorted(set(self.class_ids))

    def rows_of(self, class_id: int) -> List[int]:
        c = int(class_id)
        return [r for r, k in enumerate(self.class_ids) if k == c]

    def draw(self, classes_per_step: int, shots: int, seed: int) -> Tuple[List[int], List[int], List[int]]:
        """One episode -> (idx, seg_len, class_ids): `classes_per_step` classes chosen without replacement among those with at least
        `shots` rows, kept in ascending class id, then `shots` rows of each without replacement -- one numpy.random.RandomState(seed),
        consumed in that order.  A class with fewer rows than `shots` is never drawn."""
        n, k = int(classes_per_step), int(shots)
        if n < 1 or k < 1:
            raise ValueError(f"ROI bank: classes_per_step and shots must be at least 1, got {classes_per_step} and {shots}")
        pools = {c: self.rows_of(c) for c in self.classes()}
        able = [c for c in sorted(pools) if len(pools[c]) >= k]
        if len(able) < n:
            raise ValueError(f"ROI bank: {len(able)} classes hold at least {k} rows; an episode of {n} classes cannot be drawn")
        rng = np.random.RandomState(int(seed))
        chosen = sorted(able[i] for i in rng.choice(len(able), n, replace=False).tolist())
        idx, seg_len = [], []
        for c in chosen:
            pool = pools[c]
            idx += [pool[i] for i in rng.choice(len(pool), k, replace=False).tolist()]
            seg_len.append(k)
        return idx, seg_len, chosen


def episode_annotations(ann: Dict[str, Any], class_ids: Sequence[int]):
    """Ground truth of a query record filtered to the episode's classes and renumbered 0 .. n - 1 in the order of `class_ids`
    (meta_one_stage_detector.py:184-224) -> (boxes (m, 4), classes (m,), image_index (m,)), the order of the kept boxes unchanged."""
    bx = torch.as_tensor(ann["boxes"], dtype=torch.float32).reshape(-1, 4).cpu()
    cl = torch.as_tensor(ann["classes"]).reshape(-1).cpu().long()
    im = torch.as_tensor(ann["image_index"]).reshape(-1).cpu().long()
    if not (bx.shape[0] == cl.numel() == im.numel()):
        raise ValueError(f"train_code_generator: {bx.shape[0]} boxes, {cl.numel()} classes and {im.numel()} image indices")
    new = {int(c): j for j, c in enumerate(class_ids)}
    keep = [i for i, c in enumerate(cl.tolist()) if c in new]
    kt = torch.tensor(keep, dtype=torch.long)
    return bx[kt], torch.tensor([new[int(cl[i])] for i in keep], dtype=torch.long), im[kt]


def clip_scale(total_norm: torch.Tensor, clip_norm: Optional[float]) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_'s factor: min(1, clip_norm / (total_norm + 1e-6))"""
    if clip_norm is None:
        return torch.ones((), device=total_norm.device)
    return (float(clip_norm) / (total_norm + 1e-6)).clamp(max=1.0)


class GeneratorOptimizer(MasterSGD):
    """The generator's fp32 master copy as ONE flat device vector, with gradient clipping by total norm (the recipes set
    SOLVER.CLIP_GRADIENTS norm 1.0).  `layout` is Engine.codegen_params().  `trainable`: key prefixes; tensors no prefix matches are
    frozen and keep their bits, and they do not count in the clipped norm."""

    def __init__(self, flat: torch.Tensor, layout: Sequence[Tuple[str, int, int]], *, lr: float = 5e-4, momentum: float = 0.9,
                 weight_decay: float = 1e-4, lr_steps: Sequence[int] = (), lr_gamma: float = 0.1, clip_norm: Optional[float] = 1.0,
                 trainable: Optional[Sequence[str]] = None):
        total = layout[-1][1] + layout[-1][2]
        if flat.numel() != total:
            raise ValueError(f"GeneratorOptimizer: the flat vector holds {flat.numel()} floats, the layout {total}")
        self.p = flat.detach().to(torch.float32).reshape(-1).clone()
        self.layout = [(k, int(o), int(n)) for k, o, n in layout]
        self.clip_norm = clip_norm
        self.mask = None
        self._init_sgd([self.p], lr=lr, momentum=momentum, weight_decay=weight_decay, lr_steps=lr_steps, lr_gamma=lr_gamma)
        if trainable is not None:
            pre = tuple(trainable)
            m = torch.zeros(total, dtype=torch.bool)
            hit = set()
            for k, o, n in self.layout:
                for q in pre:
                    if k.startswith(q):
                        m[o:o + n] = True
                        hit.add(q)
            if len(hit) != len(set(pre)):
                raise ValueError(f"GeneratorOptimizer: trainable prefix {sorted(set(pre) - hit)} matches no tensor of the layout")
            if not bool(m.all()):
                self.mask = m.to(self.p.device)
                self._freeze(self.p, ~m)

    def step(self, grad_sum: torch.Tensor, num_pos: torch.Tensor):
        """grad_sum: the flat gradient of the un-normalised loss sum; divided by max(num_pos, 1) (fcos_outputs.py:651, one rank), clipped, stepped"""
        norm = num_pos.reshape(()).clamp(min=1).to(torch.float32)
        g = grad_sum / norm
        if self.mask is not None:
            g = torch.where(self.mask, g, torch.zeros_like(g))
        self._sgd_step(g * clip_scale(g.norm(), self.clip_norm))
        return norm

    def state_dict(self, engine=None) -> Dict[str, torch.Tensor]:
        """the tensors under their checkpoint keys (CPU fp32)"""
        from .engine import Engine
        flat = self.p.detach().cpu()
        return {k: flat[o:o + n].reshape(Engine.codegen_param_shape(k, n)).clone() for k, o, n in self.layout}


def _refuse(cfg):
    """what train_code_generator does not implement, by name (cfg: the model's yacs config, or None for a bare engine)"""
    if cfg is None:
        return
    ml = cfg.MODEL.META_LEARN
    cg = ml.CODE_GENERATOR
    if str(cg.get("CONTRASTIVE_LOSS", "")) != "":
        raise NotImplementedError(f"train_code_generator: CODE_GENERATOR.CONTRASTIVE_LOSS {cg.CONTRASTIVE_LOSS!r} (the soft-nearest-neighbour loss) is not supported")
    if float(cg.get("DISTILLATION_LOSS_WEIGHT", 0.0)) != 0.0:
        raise NotImplementedError(f"train_code_generator: CODE_GENERATOR.DISTILLATION_LOSS_WEIGHT {cg.DISTILLATION_LOSS_WEIGHT} is not supported")
    pg = cfg.MODEL.get("PROPOSAL_GENERATOR", {})
    if "FREEZE_CLS_TOWER" in pg and not bool(pg.FREEZE_CLS_TOWER):
        raise NotImplementedError("train_code_generator: MODEL.PROPOSAL_GENERATOR.FREEZE_CLS_TOWER is False: a query record holds a frozen tower's "
                                  "output; training the cls tower is not supported")


def train_code_generator(engine_or_model, bank: RoiBank, records, annotations, *, iters: int, classes_per_step: int, shots: int,
                         records_per_step: Optional[int] = None, lr: float = 5e-4, clip_norm: Optional[float] = 1.0, momentum: float = 0.9,
                         weight_decay: float = 1e-4, lr_steps: Sequence[int] = (), lr_gamma: float = 0.1, trainable: Optional[Sequence[str]] = None,
                         seed: int = 0, init: Optional[torch.Tensor] = None):
    """Train the generator on episodes: `bank` the RoiBank of the support instances, `records` QueryRecords of the query images with
    `annotations` (per record {"boxes" (n, 4) in network-input pixels, "classes" (n,) dataset class ids as in the bank, "image_index" (n,)
    sorted}).  Per step: bank.draw(classes_per_step, shots, seed + step); codegen_train_forward; per record of the step the annotations
    filtered to the episode's classes and renumbered, load_record + fcos_targets + cls_grad, summed; divided by max(num_pos, 1);
    codegen_train_backward; one clipped SGD step.  Starts from the engine's finalized generator (or `init`, a flat vector).  Returns
    (state_dict, losses): the trained tensors under their checkpoint keys (not installed: Engine.set_code_generator does that) and the
    normalised loss of every step as one device tensor."""
    _single_rank("train_code_generator")
    _refuse(getattr(engine_or_model, "cfg", None))
    eng = getattr(engine_or_model, "engine", engine_or_model)
    if len(annotations) != len(records):
        raise ValueError(f"train_code_generator: {len(annotations)} annotations for {len(records)} records")
    layout = eng.codegen_params()
    flat0 = eng.code_generator() if init is None else torch.as_tensor(init)
    opt = GeneratorOptimizer(flat0.to(eng.device), layout, lr=lr, momentum=momentum, weight_decay=weight_decay, lr_steps=lr_steps,
                             lr_gamma=lr_gamma, clip_norm=clip_norm, trainable=trainable)
    rows = bank.tensor()
    plan = step_records(len(records), records_per_step, int(iters), seed)
    losses = torch.zeros(int(iters), device=eng.device)
    for it, recs in enumerate(plan):
        idx, seg_len, cids = bank.draw(classes_per_step, shots, int(seed) + it)
        codes = eng.codegen_train_forward(opt.p, rows, idx, seg_len)
        n = len(seg_len)
        gcodes = torch.zeros(n, 257, device=eng.device)
        loss = torch.zeros(1, device=eng.device)
        npos = torch.zeros(1, device=eng.device, dtype=torch.int32)
        for r in recs:
            bx, cl, im = episode_annotations(annotations[r], cids)
            eng.load_record(records[r])
            labels, np1 = eng.fcos_targets(bx, cl, im)
            l1, gw, gb = eng.cls_grad(labels, codes[:, :256], codes[:, 256], check_labels=False)
            gcodes[:, :256] += gw
            gcodes[:, 256] += gb
            loss += l1
            npos += np1
        grad = eng.codegen_train_backward(gcodes)
        norm = opt.step(grad, npos)
        losses[it] = (loss / norm)[0]
    return opt.state_dict(), losses
