"""COCO bbox AP on the device: the evaluator.evaluate() step of the episodic query loops (meta_learn_evaluation.py:465 hands the gathered
detections to pycocotools' COCOeval: evaluate -> accumulate -> summarize, useCats = 1).

DeviceCOCOEvaluator keeps the detections where the decode left them, as (n, 8) rows (evaluation.DET_ROW).  evaluate() orders them with two
stable torch sorts of 64-bit keys on the device (plumbing), matches them against the uploaded ground-truth table in coco_match_kernel,
accumulates precision / recall / scores in coco_accumulate_kernel (csrc/coco_eval.hip, float64 in pycocotools' operation order) and copies the
three result arrays to the host, together with one scalar that tells whether a detection named an image the ground truth does not hold.
The summary numbers are means over slices of those arrays, taken on the host."""
import json
from collections import OrderedDict
from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import torch

from .evaluation import DET_ROW, detections_to_tensor, gather_detection_rows

AREA_RNGS = [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]


def _score_pattern(score: torch.Tensor) -> torch.Tensor:
    """fp32 scores -> int64 in [0, 2^32) that ascends where the score descends (-0 as +0): the order-preserving bit pattern of -score"""
    b = (-(score + 0.0)).contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return torch.where(b >= 0x80000000, b ^ 0xFFFFFFFF, b | 0x80000000)


class DeviceCOCOEvaluator:
    """COCO bbox evaluator with detectron2's DatasetEvaluator interface (reset / process / evaluate) for
    inference_on_dataset_with_class_codes, inference_on_dataset_with_code_sets (one evaluator per set) and cache_query_dataset lists.

    gt: a COCO-format dict or the path of its json ("images", "annotations" with bbox XYWH / area / iscrowd, "categories").
    contiguous_to_dataset_id: predicted class id -> category id (default: the id itself).  max_dets: pycocotools' maxDets.
    category_subsets: {"novel": [category ids], "base": [...]} adds the twelve numbers per subset under the name's first letter (nAP, bAP, ...).
    distributed: evaluate() gathers every rank's rows first (gather_detection_rows) and every rank returns the same dict.
    engine: the sylph_amd Engine whose stream and library run the kernels (default: a context of its own, made at the first evaluate())."""

    def __init__(self, gt, contiguous_to_dataset_id: Optional[Dict[int, int]] = None, max_dets: Sequence[int] = (1, 10, 100),
                 category_subsets: Optional[Dict[str, List[int]]] = None, distributed: bool = False, engine=None):
        if isinstance(gt, str):
            with open(gt) as f:
                gt = json.load(f)
        self.max_dets = tuple(int(m) for m in max_dets)
        if not self.max_dets or list(self.max_dets) != sorted(self.max_dets) or self.max_dets[0] < 1:
            raise ValueError(f"max_dets must ascend from at least 1, got {max_dets}")
        self.distributed = bool(distributed)
        self.engine = engine
        self.iou_thrs = np.linspace(.5, .95, 10)
        self.rec_thrs = np.linspace(0, 1, 101)
        self.image_ids = sorted(int(im["id"]) for im in gt["images"])
        cats = sorted(gt["categories"], key=lambda c: c["id"])
        self.cat_ids = [int(c["id"]) for c in cats]
        self.cat_names = [str(c.get("name", c["id"])) for c in cats]
        if not self.image_ids or not self.cat_ids:
            raise ValueError("the ground truth holds no images or no categories")
        if max(self.image_ids) >= (1 << 24) or min(self.image_ids) < 0:
            raise ValueError("image ids must be in [0, 2^24): a detection row carries them in fp32")
        I, K = len(self.image_ids), len(self.cat_ids)
        if I * K >= (1 << 31) - 1:
            raise ValueError(f"{I} images x {K} categories do not fit a pair index")
        self.category_subsets = OrderedDict()
        kidx = {c: k for k, c in enumerate(self.cat_ids)}
        for name, ids in (category_subsets or {}).items():
            missing = [c for c in ids if c not in kidx]
            if missing:
                raise ValueError(f"category_subsets[{name!r}]: category ids {missing} are not in the ground truth")
            self.category_subsets[name] = sorted(kidx[c] for c in ids)
        # ground-truth table ordered by (image, category, file order)
        iidx = {im: i for i, im in enumerate(self.image_ids)}
        anns = [(iidx[int(a["image_id"])] * K + kidx[int(a["category_id"])], j, a) for j, a in enumerate(gt["annotations"])
                if int(a["category_id"]) in kidx and int(a["image_id"]) in iidx]
        anns.sort(key=lambda x: (x[0], x[1]))
        pair = np.array([x[0] for x in anns], dtype=np.int64)
        counts = np.bincount(pair, minlength=I * K) if len(anns) else np.zeros(I * K, dtype=np.int64)
        off = np.zeros(I * K + 1, dtype=np.int64)
        np.cumsum(counts, out=off[1:])
        self._gt_host = {
            "box": np.array([[float(v) for v in x[2]["bbox"]] for x in anns], dtype=np.float64).reshape(-1, 4),
            "area": np.array([float(x[2]["area"]) for x in anns], dtype=np.float64),
            "crowd": np.array([1 if x[2].get("iscrowd", 0) else 0 for x in anns], dtype=np.int32),
            "off": off.astype(np.int32),
            "max_per_pair": int(counts.max()) if len(anns) else 0,
        }
        # predicted class id -> category index (-1: no category of the ground truth)
        c2d = contiguous_to_dataset_id
        ncls = (max(c2d) + 1) if c2d else (max(self.cat_ids) + 1)
        table = np.full(max(ncls, 1), -1, dtype=np.int64)
        for c in range(ncls):
            d = c2d.get(c) if c2d else c
            if d is not None and int(d) in kidx:
                table[c] = kidx[int(d)]
        self._class_to_k_host = table
        self._dev = None  # device the tables were uploaded to
        self._rows: List[torch.Tensor] = []
        self.precision = self.recall = self.scores = None

    # ---- DatasetEvaluator -----------------------------------------------------------------------------------------------------------
    def reset(self):
        self._rows = []
        self.precision = self.recall = self.scores = None

    def process(self, inputs, outputs):
        """appends the batch's (n, 8) rows to the device list: no device -> host copy, no synchronisation"""
        self._rows.append(detections_to_tensor(outputs, [int(x["image_id"]) for x in inputs]))

    def evaluate(self):
        rows = [r for r in self._rows if r.shape[0]]
        dev = rows[0].device if rows else (self._rows[0].device if self._rows else self._default_device())
        rows = torch.cat(rows) if rows else torch.zeros(0, DET_ROW, device=dev)
        if self.distributed:
            rows = self._gather(rows)
        engine = self._engine(dev)
        prep = self._order(rows)
        gt = self._tables(dev)
        matched, ignored, npig = engine.coco_match(prep["rows"], prep["det_off"], gt, len(self.cat_ids), gt["iou_thrs"], gt["area_rngs"],
                                                   self.max_dets[-1])
        p2 = prep["perm2"]
        precision, recall, scores = engine.coco_accumulate(prep["rows"][:, 5][p2].contiguous(), prep["rank"][p2], matched[p2], ignored[p2],
                                                           prep["cat_off"], npig, len(self.iou_thrs), gt["rec_thrs"], gt["max_dets"])
        self.precision, self.recall, self.scores = precision.cpu().numpy(), recall.cpu().numpy(), scores.cpu().numpy()
        bad = float(prep["bad_id"].cpu())
        if bad >= 0:
            raise ValueError(f"detection on image id {int(bad)}, which the ground truth does not hold")
        return OrderedDict(bbox=self._summarize())

    # ---- plumbing: torch on the device, nothing read back ------------------------------------------------------------------------------
    def _order(self, rows: torch.Tensor) -> Dict[str, torch.Tensor]:
        """rows ordered by (pair, score descending, arrival) with the pairs' offsets and ranks, and the permutation that orders those by
        (category, score descending): image ascending, then rank, among equal scores of a category."""
        dev = rows.device
        gt = self._tables(dev)
        I, K = len(self.image_ids), len(self.cat_ids)
        n = rows.shape[0]
        ids = rows[:, 0].contiguous()
        img = torch.searchsorted(gt["image_ids"], ids).clamp_(max=I - 1)
        known = gt["image_ids"][img] == ids
        valid = rows[:, 7] > 0
        cls = rows[:, 6].to(torch.int64)
        in_table = (cls >= 0) & (cls < gt["class_to_k"].numel())
        k = gt["class_to_k"][cls.clamp(0, gt["class_to_k"].numel() - 1)]
        use = valid & known & in_table & (k >= 0)
        pair = torch.where(use, img * K + k, torch.full_like(img, I * K))
        minus_one = torch.full((1,), -1.0, device=dev)
        bad_id = torch.cat([torch.where(valid & ~known, ids, minus_one.expand(n)), minus_one]).max()  # -1: every image id is known
        pattern = _score_pattern(rows[:, 5])
        perm1 = torch.sort((pair << 32) | pattern, stable=True).indices
        rows1, pair1 = rows[perm1].contiguous(), pair[perm1]
        det_off = torch.searchsorted(pair1, torch.arange(I * K + 1, device=dev))
        rank = torch.arange(n, device=dev) - det_off[pair1.clamp(max=I * K - 1)]
        cat1 = torch.where(pair1 < I * K, pair1 % K, torch.full_like(pair1, K))
        key2 = (cat1 << 32) | pattern[perm1]
        perm2 = torch.sort(key2, stable=True).indices
        cat_off = torch.searchsorted(cat1[perm2].contiguous(), torch.arange(K + 1, device=dev))
        return {"rows": rows1, "det_off": det_off.to(torch.int32), "rank": rank.to(torch.int32), "perm2": perm2,
                "cat_off": cat_off.to(torch.int32), "bad_id": bad_id}

    def _tables(self, dev) -> Dict[str, Any]:
        if self._dev != dev:  # uploaded once per device
            h = self._gt_host
            self._tab = {
                "box": torch.from_numpy(h["box"]).to(dev), "area": torch.from_numpy(h["area"]).to(dev),
                "crowd": torch.from_numpy(h["crowd"]).to(dev), "off": torch.from_numpy(h["off"]).to(dev), "max_per_pair": h["max_per_pair"],
                "image_ids": torch.tensor(self.image_ids, dtype=torch.float32, device=dev),
                "class_to_k": torch.from_numpy(self._class_to_k_host).to(dev),
                "iou_thrs": torch.from_numpy(self.iou_thrs).to(dev), "rec_thrs": torch.from_numpy(self.rec_thrs).to(dev),
                "area_rngs": torch.tensor(AREA_RNGS, dtype=torch.float64, device=dev),
                "max_dets": torch.tensor(self.max_dets, dtype=torch.int32, device=dev),
            }
            self._dev = dev
        return self._tab

    def _gather(self, rows: torch.Tensor) -> torch.Tensor:
        """one gather_detection_rows; the block size is the largest per-rank count: one all_reduce of a device scalar, read back because
        the block size is a host int (the only read-back before the results, and only with distributed=True)"""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return rows
        cap = torch.tensor([rows.shape[0]], device=rows.device)
        dist.all_reduce(cap, op=dist.ReduceOp.MAX)
        return gather_detection_rows(rows, max(int(cap), 1))

    def _default_device(self):
        return self.engine.device if self.engine is not None else torch.device("cuda", torch.cuda.current_device())

    def _engine(self, dev):
        if self.engine is None:
            from .engine import Engine
            self.engine = Engine(None, dtype="f32", device=dev.index if dev.index is not None else 0)
        return self.engine

    # ---- summaries: means over slices of the host arrays ------------------------------------------------------------------------------------
    @staticmethod
    def _mean(s: np.ndarray) -> float:
        s = s[s > -1]
        return float(np.mean(s)) if s.size else -1.0

    def _twelve(self, ksel) -> "OrderedDict[str, float]":
        p, r = self.precision[:, :, ksel], self.recall[:, ksel]
        out = OrderedDict()
        out["AP"] = self._mean(p[:, :, :, 0, -1])
        out["AP50"] = self._mean(p[0, :, :, 0, -1])
        out["AP75"] = self._mean(p[5, :, :, 0, -1])
        for a, n in ((1, "s"), (2, "m"), (3, "l")):
            out["AP" + n] = self._mean(p[:, :, :, a, -1])
        for m, md in enumerate(self.max_dets):
            out[f"AR@{md}"] = self._mean(r[:, :, 0, m])
        for a, n in ((1, "s"), (2, "m"), (3, "l")):
            out["AR" + n] = self._mean(r[:, :, a, -1])
        return out

    def _summarize(self) -> "OrderedDict[str, float]":
        """detectron2's _derive_coco_results: x 100, NaN where a slice has no entry; AP-<name> per category; the subsets' numbers"""
        pct = lambda v: v * 100 if v >= 0 else float("nan")
        out = OrderedDict((k, pct(v)) for k, v in self._twelve(slice(None)).items())
        for k, name in enumerate(self.cat_names):
            out["AP-" + name] = pct(self._mean(self.precision[:, :, k, 0, -1]))
        for name, ks in self.category_subsets.items():
            for key, v in self._twelve(ks).items():
                out[name[0] + key] = pct(v)
        return out
