"""LVIS (federated) bbox AP on the device: the evaluator.evaluate() step of the episodic query loops for the two LVIS v1 configurations.
The reference scores them with FewshotLVISEvaluator (sylph/evaluation/lvis_evaluation.py), which hands the detections to lvis-api's
LVISResults + LVISEval; this module follows that protocol for iou_type "bbox" and is pinned to tests/lviseval_ref.py, a float64 numpy
restatement of it -- not to lvis-api itself, which is not compared against anywhere in this repository.

DeviceLVISEvaluator keeps the detections as (n, 8) device rows, exactly as DeviceCOCOEvaluator does.  evaluate() runs the per-image budget,
the class -> category map, the federated membership test and the list of the (image, category) pairs that exist as torch sorts /
searchsorted / cumsum on the device (plumbing; pair keys are int64 and no table of images x categories is ever built), matches the pairs in
lvis_match_kernel (csrc/lvis_eval.hip) and accumulates with coco_accumulate_kernel (one unbounded maxDet), a slab of categories per launch so
that the result slabs stay small on the device.  Nothing is copied to the host before the result arrays and the one unknown-image scalar."""
import json
from collections import OrderedDict
from typing import Any, Dict, Iterable, List, Optional

import numpy as np
import torch

from ._lib import LVIS_MATCH_MAX_DETS
from .coco_eval import AREA_RNGS, DeviceCOCOEvaluator, _score_pattern
from .evaluation import DET_ROW

ACC_SLAB = 256  # categories per sylph_coco_accumulate launch: 2 x 8.3 MB of float64 results on the device at a time
METRICS = ("AP", "AP50", "AP75", "APs", "APm", "APl", "APr", "APc", "APf")


def short_name(x: str) -> str:
    """the reference's per-category key (lvis_evaluation.py:282-289)"""
    return x[:11] + ".." if len(x) > 13 else x


def _member(table: torch.Tensor, key: torch.Tensor) -> torch.Tensor:
    """key in table; table: sorted int64 that ends with a sentinel no key equals"""
    return table[torch.searchsorted(table, key).clamp_(max=table.numel() - 1)] == key


class DeviceLVISEvaluator(DeviceCOCOEvaluator):
    """LVIS bbox evaluator with detectron2's DatasetEvaluator interface (reset / process / evaluate) for
    inference_on_dataset_with_class_codes, inference_on_dataset_with_code_sets (one evaluator per set) and cache_query_dataset lists.

    gt: an LVIS-format dict or the path of its json: "images" with neg_category_ids / not_exhaustive_category_ids (default []), "annotations"
    with bbox XYWH / area / optional ignore, "categories" with optional frequency "r" | "c" | "f".
    contiguous_to_dataset_id: predicted class id -> category id (default: the id itself; None: a class with no category, which still uses
    up its image's budget).  category_ids: keep only these categories, their annotations and the images that hold one of those
    (FewshotLVIS._create_index); a detection on any other image is an error.  max_dets_per_image: LVISResults' budget over all categories.
    category_subsets: {"novel": [category ids], ...} adds the nine numbers per subset under the name's first letter (nAP, ..., nAPf).
    distributed / engine: as for DeviceCOCOEvaluator.  The result is OrderedDict(bbox=...) with the reference's numbers: the nine metrics x 100
    (an empty slice reads -100.0) and AP-<short name> per category (NaN without ground truth); .precision [T, R, K, A] and .recall [T, K, A]."""

    def __init__(self, gt, contiguous_to_dataset_id: Optional[Dict[int, int]] = None, category_ids: Optional[Iterable[int]] = None,
                 max_dets_per_image: int = 300, category_subsets: Optional[Dict[str, List[int]]] = None, distributed: bool = False, engine=None):
        if isinstance(gt, str):
            with open(gt) as f:
                gt = json.load(f)
        self.max_dets_per_image = int(max_dets_per_image)
        if self.max_dets_per_image < 1:
            raise ValueError(f"max_dets_per_image must be at least 1, got {max_dets_per_image}")
        if self.max_dets_per_image > LVIS_MATCH_MAX_DETS:
            raise ValueError(f"max_dets_per_image {max_dets_per_image} is over LVIS_MATCH_MAX_DETS = {LVIS_MATCH_MAX_DETS}: a pair may hold every "
                             "detection of its image, and the match kernel keeps their boxes on chip")
        self.distributed = bool(distributed)
        self.engine = engine
        self.iou_thrs = np.linspace(.5, .95, 10)
        self.rec_thrs = np.linspace(0, 1, 101)
        keep = None if category_ids is None else {int(c) for c in category_ids}
        cats = sorted((c for c in gt["categories"] if keep is None or int(c["id"]) in keep), key=lambda c: c["id"])
        self.cat_ids = [int(c["id"]) for c in cats]
        self.cat_names = [str(c.get("name", c["id"])) for c in cats]
        kidx = {c: k for k, c in enumerate(self.cat_ids)}
        anns = [(j, a) for j, a in enumerate(gt["annotations"]) if int(a["category_id"]) in kidx]
        with_ann = {int(a["image_id"]) for _, a in anns}
        images = [im for im in gt["images"] if keep is None or int(im["id"]) in with_ann]
        self.image_ids = sorted(int(im["id"]) for im in images)
        if not self.image_ids or not self.cat_ids:
            raise ValueError("the ground truth holds no images or no categories")
        if max(self.image_ids) >= (1 << 24) or min(self.image_ids) < 0:
            raise ValueError("image ids must be in [0, 2^24): a detection row carries them in fp32")
        I, K = len(self.image_ids), len(self.cat_ids)
        iidx = {im: i for i, im in enumerate(self.image_ids)}
        self.freq_groups = {f: [k for k, c in enumerate(cats) if c.get("frequency") == f] for f in "rcf"}
        self.category_subsets = OrderedDict()
        for name, ids in (category_subsets or {}).items():
            missing = [c for c in ids if c not in kidx]
            if missing:
                raise ValueError(f"category_subsets[{name!r}]: category ids {missing} are not in the ground truth")
            self.category_subsets[name] = sorted(kidx[c] for c in ids)
        # ground-truth table ordered by (pair key, file order); pair key = image index * K + category index, int64
        table = sorted((iidx[int(a["image_id"])] * K + kidx[int(a["category_id"])], j, a) for j, a in anns if int(a["image_id"]) in iidx)
        key = np.array([x[0] for x in table], dtype=np.int64)
        gt_keys, counts = np.unique(key, return_counts=True)
        pair_off = np.zeros(len(gt_keys) + 1, dtype=np.int64)
        np.cumsum(counts, out=pair_off[1:])
        allowed, not_exh = set(gt_keys.tolist()), set()
        for im in images:
            i = iidx[int(im["id"])]
            allowed.update(i * K + kidx[int(c)] for c in im.get("neg_category_ids", []) if int(c) in kidx)
            not_exh.update(i * K + kidx[int(c)] for c in im.get("not_exhaustive_category_ids", []) if int(c) in kidx)
        big = I * K  # no pair key reaches it: the sentinel of dropped rows and the tables' last entry
        self._gt_host = {
            "box": np.array([[float(v) for v in x[2]["bbox"]] for x in table], dtype=np.float64).reshape(-1, 4),
            "area": np.array([float(x[2]["area"]) for x in table], dtype=np.float64),
            "ignore": np.array([1 if x[2].get("ignore", 0) else 0 for x in table], dtype=np.int32),
            "keys": gt_keys.astype(np.int64), "pair_off": pair_off,
            "allowed": np.array(sorted(allowed) + [big], dtype=np.int64), "not_exh": np.array(sorted(not_exh) + [big], dtype=np.int64),
            "max_per_pair": int(counts.max()) if len(table) else 0,
        }
        c2d = contiguous_to_dataset_id
        ncls = (max(c2d) + 1) if c2d else (max(self.cat_ids) + 1)
        cls_table = np.full(max(ncls, 1), -1, dtype=np.int64)
        for c in range(ncls):
            d = c2d.get(c) if c2d else c
            if d is not None and int(d) in kidx:
                cls_table[c] = kidx[int(d)]
        self._class_to_k_host = cls_table
        self._dev = None
        self._rows: List[torch.Tensor] = []
        self.precision = self.recall = None

    def reset(self):
        self._rows = []
        self.precision = self.recall = None

    def evaluate(self):
        rows = [r for r in self._rows if r.shape[0]]
        dev = rows[0].device if rows else (self._rows[0].device if self._rows else self._default_device())
        rows = torch.cat(rows) if rows else torch.zeros(0, DET_ROW, device=dev)
        if self.distributed:
            rows = self._gather(rows)
        engine = self._engine(dev)
        prep = self._order(rows)
        gt = self._tables(dev)
        K, T = len(self.cat_ids), len(self.iou_thrs)
        matched, ignored, npig = engine.lvis_match(prep["rows"], prep["pairs"], gt, K, gt["iou_thrs"], gt["area_rngs"], self.max_dets_per_image)
        p2 = prep["perm2"]
        score, rank, matched, ignored = prep["rows"][:, 5][p2].contiguous(), prep["rank"][p2], matched[p2], ignored[p2]
        precision = np.empty((T, len(self.rec_thrs), K, len(AREA_RNGS)))
        recall = np.empty((T, K, len(AREA_RNGS)))
        for k0 in range(0, K, ACC_SLAB):  # the COCO accumulation with one unbounded maxDet; its scores array is not used
            k1 = min(K, k0 + ACC_SLAB)
            p, r, _ = engine.coco_accumulate(score, rank, matched, ignored, prep["cat_off"][k0:k1 + 1].contiguous(), npig[k0:k1].contiguous(), T,
                                             gt["rec_thrs"], gt["max_dets"])
            precision[:, :, k0:k1], recall[:, k0:k1] = p[..., 0].cpu().numpy(), r[..., 0].cpu().numpy()
            del p, r, _
        self.precision, self.recall = precision, recall
        bad = float(prep["bad_id"].cpu())
        if bad >= 0:
            raise ValueError(f"detection on image id {int(bad)}, which the ground truth does not hold")
        return OrderedDict(bbox=self._summarize())

    # ---- plumbing: torch on the device, nothing read back ------------------------------------------------------------------------------
    def _order(self, rows: torch.Tensor) -> Dict[str, Any]:
        """the rows LVIS uses -- inside their image's budget, of a kept category that is positive or negative there -- ordered by (pair, score
        descending, arrival), the dropped ones behind them; the compacted list of the pairs that exist (from detections or ground truth) in
        ascending key order with their offsets, categories and flags, sized by the host-known bound rows + ground-truth pairs with the live
        count as a device scalar; and the permutation that orders the rows by (category, score descending, image, rank)."""
        dev = rows.device
        gt = self._tables(dev)
        I, K = len(self.image_ids), len(self.cat_ids)
        big = I * K
        n = rows.shape[0]
        ar = lambda m: torch.arange(m, device=dev)
        ids = rows[:, 0].contiguous()
        img = torch.searchsorted(gt["image_ids"], ids).clamp_(max=I - 1)
        known = gt["image_ids"][img] == ids
        valid = rows[:, 7] > 0
        minus_one = torch.full((1,), -1.0, device=dev)
        bad_id = torch.cat([torch.where(valid & ~known, ids, minus_one.expand(n)), minus_one]).max()  # -1: every image id is known
        # per-image budget: (image, score descending, arrival), rank inside the image, before any category filtering
        img = torch.where(valid & known, img, torch.full_like(img, I))
        pattern = _score_pattern(rows[:, 5])
        perm0 = torch.sort((img << 32) | pattern, stable=True).indices
        img0, rows0, pattern0 = img[perm0], rows[perm0], pattern[perm0]
        img_off = torch.searchsorted(img0, ar(I + 1))
        in_budget = (ar(n) - img_off[img0]) < self.max_dets_per_image
        # class -> category, federated membership
        cls = rows0[:, 6].to(torch.int64)
        in_table = (cls >= 0) & (cls < gt["class_to_k"].numel())
        k = gt["class_to_k"][cls.clamp(0, gt["class_to_k"].numel() - 1)]
        key = img0 * K + k
        use = (img0 < I) & in_budget & in_table & (k >= 0) & _member(gt["allowed"], key)
        key = torch.where(use, key, torch.full_like(key, big))
        perm1 = torch.sort(key, stable=True).indices  # stable: (score descending, arrival) survives inside a pair
        key1, rows1, pattern1 = key[perm1], rows0[perm1].contiguous(), pattern0[perm1]
        # the pairs that exist: distinct keys of the used rows and of the ground truth
        P = max(n + gt["keys"].numel(), 1)
        s, o = torch.sort(torch.cat([key1, gt["keys"]]), stable=True)
        new = (s != torch.cat([torch.full((1,), -1, dtype=torch.int64, device=dev), s])[:-1]) & (s < big)
        pidx_s = torch.cumsum(new, 0) - 1
        pidx = torch.empty_like(pidx_s)
        pidx[o] = torch.where(s < big, pidx_s, torch.full_like(s, P))
        pd, pg = pidx[:n], pidx[n:]  # pair index of every row (P: dropped) and of every ground-truth pair
        pair_key = torch.full((P + 1,), big, dtype=torch.int64, device=dev)
        pair_key.scatter_(0, torch.where(new, pidx_s, torch.full_like(s, P)), s)  # slot P takes the repeats
        pair_key = pair_key[:P]
        det_off = torch.searchsorted(pd.contiguous(), ar(P + 1))
        rank = ar(n) - det_off[pd]
        gt_off = gt["pair_off"][torch.searchsorted(pg.contiguous(), ar(P + 1))]
        pairs = {"n": new.sum().to(torch.int32).reshape(1), "cat": (pair_key % K).to(torch.int32),
                 "flags": _member(gt["not_exh"], pair_key).to(torch.int32), "det_off": det_off.to(torch.int32), "gt_off": gt_off.to(torch.int32)}
        cat1 = torch.where(key1 < big, key1 % K, torch.full_like(key1, K))
        perm2 = torch.sort((cat1 << 32) | pattern1, stable=True).indices
        cat_off = torch.searchsorted(cat1[perm2].contiguous(), ar(K + 1))
        return {"rows": rows1, "pairs": pairs, "pair_key": pair_key, "rank": rank.to(torch.int32), "perm2": perm2,
                "cat_off": cat_off.to(torch.int32), "bad_id": bad_id}

    def _tables(self, dev) -> Dict[str, Any]:
        if self._dev != dev:  # uploaded once per device
            h = self._gt_host
            up = lambda a: torch.from_numpy(a).to(dev)
            self._tab = {
                "box": up(h["box"]), "area": up(h["area"]), "ignore": up(h["ignore"]), "keys": up(h["keys"]), "pair_off": up(h["pair_off"]),
                "allowed": up(h["allowed"]), "not_exh": up(h["not_exh"]), "max_per_pair": h["max_per_pair"],
                "image_ids": torch.tensor(self.image_ids, dtype=torch.float32, device=dev), "class_to_k": up(self._class_to_k_host),
                "iou_thrs": up(self.iou_thrs), "rec_thrs": up(self.rec_thrs),
                "area_rngs": torch.tensor(AREA_RNGS, dtype=torch.float64, device=dev),
                "max_dets": torch.tensor([self.max_dets_per_image], dtype=torch.int32, device=dev),
            }
            self._dev = dev
        return self._tab

    # ---- summaries: means over slices of the host arrays ------------------------------------------------------------------------------------
    def _nine(self, ks: List[int]) -> "OrderedDict[str, float]":
        """LVISEval._summarize over the category indices ks, x 100 as the reference reports them: an empty slice reads -100.0"""
        p = self.precision
        out = OrderedDict()
        out["AP"] = self._mean(p[:, :, ks, 0])
        out["AP50"] = self._mean(p[0][:, ks, 0])
        out["AP75"] = self._mean(p[5][:, ks, 0])
        for a, n in ((1, "s"), (2, "m"), (3, "l")):
            out["AP" + n] = self._mean(p[:, :, ks, a])
        for f in "rcf":
            group = set(self.freq_groups[f])
            out["AP" + f] = self._mean(p[:, :, [k for k in ks if k in group], 0])
        return OrderedDict((k, float(v * 100)) for k, v in out.items())

    def _summarize(self) -> "OrderedDict[str, float]":
        out = self._nine(list(range(len(self.cat_ids))))
        per_cat = OrderedDict()
        for k, name in enumerate(self.cat_names):  # a later category overwrites an equal short name, as the reference's dict.update does
            s = self.precision[:, :, k, 0]
            s = s[s > -1]
            per_cat["AP-" + short_name(name)] = float(np.mean(s) * 100) if s.size else float("nan")
        out.update(per_cat)
        for name, ks in self.category_subsets.items():
            for key, v in self._nine(ks).items():
                out[name[0] + key] = v
        return out
