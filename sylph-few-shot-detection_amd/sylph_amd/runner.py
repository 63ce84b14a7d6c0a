"""MetaFCOSRunner: the reference's orchestration/plugin point for this path
(sylph/runner/meta_fcos_runner.py:92-701), reduced to inference: get_default_cfg, build_model,
_gather_class_code and the meta-test control flow of _do_test_meta_learning.  Dataset registration,
evaluators and training are out of scope: loaders are passed in (or synthetic)."""
import importlib
import logging
import os
from collections import OrderedDict
from typing import Any, Dict, List, Optional

import torch

from . import config as _config
from . import distributed as D
from .evaluation import (cache_query_dataset, class_codes_from_bank, format_class_codes_shared, inference_normalization, inference_on_dataset_with_class_codes,
                         inference_on_dataset_with_code_sets, inference_on_support_set_dataset, inference_on_support_set_dataset_base,
                         release_query_records)
from .modeling import build_model as _build_model

logger = logging.getLogger(__name__)


def create_runner(class_full_name: str, *args, **kwargs):
    """d2go.runner.create_runner: dotted path -> instance ("sylph_amd.runner.MetaFCOSRunner"; the
    reference's own "sylph.runner.MetaFCOSRunner" is accepted and rerouted here)."""
    if class_full_name.startswith("sylph.runner."):
        class_full_name = "sylph_amd.runner." + class_full_name[len("sylph.runner."):]
    module_name, _, cls_name = class_full_name.rpartition(".")
    cls = getattr(importlib.import_module(module_name), cls_name)
    return cls(*args, **kwargs)


def create_cfg(default_cfg, config_file: Optional[str], overwrite_opts: Optional[List[Any]] = None):
    """tools/setup.py:190-209 create_cfg_from_cli_args core: defaults <- yaml (sylph:// ok) <- opts."""
    cfg = default_cfg.clone()
    if config_file:
        cfg.merge_from_file(config_file)
    if overwrite_opts:
        cfg.merge_from_list(overwrite_opts)
    return cfg


def _rows_from_codes(codes: List[Dict[str, Any]], device) -> torch.Tensor:
    """list of {"support_set_target", "class_name", "class_code": {...}} -> packed rows (sylph_amd.distributed layout)."""
    if not codes:
        return torch.zeros(0, D.ROW, device=device)
    for c in codes:
        D.require_1x1_codes(c["class_code"]["cls_conv"], "_rows_from_codes")
    conv = torch.cat([c["class_code"]["cls_conv"].reshape(1, 256).float() for c in codes]).to(device)
    bias = torch.cat([c["class_code"]["cls_bias"].reshape(1).float() for c in codes]).to(device)
    acc = [float(c["class_code"].get("acc_weight", 1.0)) for c in codes]
    has_acc = [float("acc_weight" in c["class_code"]) for c in codes]
    has_wn = all("cls_weight_norm" in c["class_code"] for c in codes)
    wn = torch.cat([c["class_code"]["cls_weight_norm"].reshape(1).float() for c in codes]).to(device) if has_wn else None
    return D.pack_codes(conv, bias, [int(c["support_set_target"]) for c in codes], acc, wn,
                        [c.get("class_name") for c in codes], has_acc=has_acc)


def _codes_from_rows(rows: torch.Tensor, keep_acc: Optional[bool], extras: Dict[int, Dict[str, Any]] = None) -> List[Dict[str, Any]]:
    """Valid packed rows (host) -> the reference's list-of-dicts form, in row order.  keep_acc None: a row gets its "acc_weight" key
    back iff the record it was packed from carried one (the explicit F_HAS_ACC lane, not a guess from the value)."""
    rows = rows.cpu()
    rows = rows[rows[:, D.F_VALID] > 0]
    names = D.unpack_names(rows)
    out = []
    for r, name in zip(rows, names):
        cid = int(round(float(r[D.F_CID])))
        cc = {"cls_conv": r[:256].reshape(1, 256, 1, 1).clone(), "cls_bias": r[256:257].reshape(1, 1, 1, 1).clone()}
        if float(r[D.F_HAS_WNORM]) > 0:
            cc["cls_weight_norm"] = r[D.F_WNORM:D.F_WNORM + 1].reshape(1, 1, 1, 1).clone()
        if keep_acc or (keep_acc is None and float(r[D.F_HAS_ACC]) > 0):
            cc["acc_weight"] = float(r[D.F_ACC])
        rec = dict(extras.get(cid, {})) if extras else {}
        rec.update({"support_set_target": cid, "class_name": rec.get("class_name") or name, "class_code": cc})
        out.append(rec)
    return out


def reduce_class_code(out_codes: List[Dict], engine=None) -> List[Dict]:
    """sylph/modeling/code_generator/utils.py:397-427 on the dict form.  With an Engine the sums run on the GPU
    (sylph_reduce_codes, fixed row order); without one (CPU-only unit tests) on host rows with the same arithmetic."""
    if len(out_codes) == 0:
        return out_codes
    assert "class_code" in out_codes[0]
    others = {}
    for c in out_codes:
        others.setdefault(int(c["support_set_target"]), {k: v for k, v in c.items() if k != "class_code"})
    if engine is not None:
        rows = _rows_from_codes(out_codes, engine.device)
        ncls = max(others) + 1
        red = engine.reduce_codes(rows.contiguous(), ncls).cpu()
        first = list(dict.fromkeys(int(c["support_set_target"]) for c in out_codes))  # the reference keeps first-appearance order
        red = red[torch.tensor(first, dtype=torch.long)]
    else:
        red = D.reduce_packed_codes(_rows_from_codes(out_codes, torch.device("cpu")))
    return _codes_from_rows(red, keep_acc=False, extras=others)


class MetaFCOSRunner:
    def __init__(self):
        self._logger = logging.getLogger(__name__)

    def get_default_cfg(self):
        """meta_fcos_runner.py:104-114."""
        return _config.get_default_cfg()

    def build_model(self, cfg, eval_only: bool = False, dtype: Optional[str] = None):
        """d2go GeneralizedRCNNRunner.build_model: registry lookup + optional MODEL.WEIGHTS load."""
        model = _build_model(cfg, dtype=dtype)
        if cfg.MODEL.WEIGHTS and os.path.exists(str(cfg.MODEL.WEIGHTS)):
            model.load_checkpoint(str(cfg.MODEL.WEIGHTS))
        if eval_only:
            model.eval()
        return model

    @classmethod
    def _gather_class_code(cls, sub_class_codes: List[Dict[str, Any]], reduce: bool = False, capacity: Optional[int] = None,
                           engine=None) -> List[Dict[str, Any]]:
        """meta_fcos_runner.py:381-439.  Same result as all_gather_object + rank-order flatten, but everything a code
        carries (weights, bias, accumulated weight + whether the record had one, class id, weight norm, class name) travels in
        ONE dense fp32 block per rank through ONE all_gather_into_tensor over RCCL / gloo (sylph_amd.distributed): no pickle,
        no count exchange, no device read-back before the rows become host dicts again.  `capacity` = rows every rank reserves
        (`_episode` derives it from the loader's global length -- the InferenceSampler shard size ceil(n / world), known on every
        rank without communication); a bare call without it agrees on one with a scalar all_reduce(MAX) of the local counts.
        A rank holding more rows than `capacity` does not raise in front of the collective (the other ranks would hang in it): the
        overflow travels in the block and EVERY rank raises distributed.GatherOverflow afterwards."""
        world = D.get_world_size()
        if world > 1:
            import torch.distributed as dist
            dev = sub_class_codes[0]["class_code"]["cls_conv"].device if sub_class_codes else torch.device("cpu")
            if dist.get_backend() == "nccl":
                dev = torch.device("cuda", torch.cuda.current_device())
            local = _rows_from_codes(sub_class_codes, dev)
            if capacity is None:
                cap = torch.tensor([local.shape[0]], dtype=torch.int64, device=dev)
                dist.all_reduce(cap, op=dist.ReduceOp.MAX)
                capacity = max(int(cap.item()), 1)
            capacity = max(int(capacity), 1)  # as gather_packed_codes / fit_block clamp it: a zero-row block cannot carry the overflow flag
            rows = D.gather_packed_codes(local, capacity).cpu()
            D.check_overflow(rows, capacity)  # same decision on every rank, after the collective
            # "acc_weight" comes back on exactly the records that carried it (explicit flag lane): nothing is inferred from values
            out_codes = _codes_from_rows(rows, keep_acc=None)
        else:
            out_codes = sub_class_codes
        if not reduce:
            return out_codes
        return reduce_class_code(out_codes, engine=engine)

    # ---- loaders: dataset registration is out of scope; a deployment overrides these three --------------------------
    def build_episodic_learning_detection_test_support_set_loader(self, cfg, dataset_name: str, seed: int = 0):
        """meta_fcos_runner.py:241-259 -> loop A's loader (one class per item) for (dataset, seed)."""
        raise NotImplementedError("dataset registration/loading (sylph/data/*) is out of scope: override this builder or pass "
                                  "support_loader / loaders= to _do_test_meta_learning")

    def build_episodic_learning_detection_test_support_set_base_loader(self, cfg, dataset_name: str):
        """meta_fcos_runner.py:261-279 -> the base-class all-ground-truth chunk loader (USE_ALL_GTS_IN_BASE_CLASSES)."""
        raise NotImplementedError("override build_episodic_learning_detection_test_support_set_base_loader")

    def build_episodic_learning_detection_test_query_loader(self, cfg, dataset_name: str):
        """meta_fcos_runner.py:281-296 -> loop B's loader."""
        raise NotImplementedError("override build_episodic_learning_detection_test_query_loader")

    def get_evaluator(self, cfg, dataset_name: str, output_folder: Optional[str] = None):
        """None = the no-op evaluator of inference_on_dataset_with_class_codes.  Dataset registration is out of scope, so no ground truth is
        known here; an override returns sylph_amd.coco_eval.DeviceCOCOEvaluator(gt json, ...) for COCO bbox AP, or, for an LVIS dataset (the
        reference's FewshotLVISEvaluator), sylph_amd.lvis_eval.DeviceLVISEvaluator(gt json, contiguous_to_dataset_id=..., category_ids=...)
        for the federated LVIS bbox AP with APr / APc / APf."""
        return None

    @staticmethod
    def _global_len(loader, fallback: Optional[int] = None) -> Optional[int]:
        """Items of a loader over ALL ranks (the synthetic loaders expose `num_items`; torch DataLoaders their dataset)."""
        for attr in ("num_items",):
            if hasattr(loader, attr):
                return int(getattr(loader, attr))
        ds = getattr(loader, "dataset", None)
        if ds is not None and hasattr(ds, "__len__"):
            return len(ds)
        return fallback

    def _episode_codes(self, cfg, model, support_loader, base_support_loader=None, output_folder: Optional[str] = None,
                       num_classes: Optional[int] = None):
        """The support half of ONE (dataset, seed) of meta_fcos_runner.py:497-560: support codes -> gather -> (base-class reduce +
        replace) -> normalise -> the formatted class codes the query loop takes."""
        sub = inference_on_support_set_dataset(model, support_loader, output_dir=output_folder)
        n_items = self._global_len(support_loader, num_classes)
        codes = self._gather_class_code(sub, capacity=D.shard_capacity(n_items) if n_items else None)
        if base_support_loader is not None:
            base_sub = inference_on_support_set_dataset_base(model, base_support_loader)
            # the base path delivers at most one accumulated row per class and rank
            n_base = num_classes if num_classes else self._global_len(base_support_loader)
            base = self._gather_class_code(base_sub, reduce=True, engine=getattr(model, "engine", None), capacity=n_base)
            by_cid = {int(c["support_set_target"]): c for c in base}
            codes = [dict(c, class_code=by_cid[int(c["support_set_target"])]["class_code"])
                     if int(c["support_set_target"]) in by_cid else c for c in codes]  # replace_class_code
        if str(cfg.MODEL.META_LEARN.CODE_GENERATOR.NAME) != "ROIEncoder":
            codes = inference_normalization(model, codes)  # ROIEncoder codes need none (and the reference call raises)
        if num_classes is not None:
            assert len(codes) == num_classes, \
                f"Got {len(codes)} class codes for prediction, but expect to be {num_classes}."
        return format_class_codes_shared(codes, device=model.device)

    @staticmethod
    def _support_batch(support_loader):
        """every support record of the loader as an annotated image: its boxes labelled with its item's support_set_target"""
        batch = []
        for item in support_loader:
            for x in item:
                c = int(x["support_set_target"])
                for rec in x["support_set"]:
                    src = rec["instances"]
                    inst = type(src)(src.image_size)
                    inst.gt_boxes = src.gt_boxes
                    inst.gt_classes = torch.full((len(src.gt_boxes),), c, dtype=torch.long)
                    batch.append(dict({k: v for k, v in rec.items() if k != "instances"}, instances=inst))
        return batch

    @staticmethod
    def _finetune_box_branch(model, support_loader, box_branch: Dict[str, Any]):
        """The box half of the tfa-finetune recipe for one (dataset, seed): the box branch trained on that seed's support images
        (MetaOneStageDetector.finetune_box_branch; box_branch: its keyword arguments).  Returns the branch; the caller installs it."""
        kw = dict(box_branch)
        kw.setdefault("batch_size", 16)
        batch = MetaFCOSRunner._support_batch(support_loader)
        branch, losses = model.finetune_box_branch(batch, **kw)
        ls = losses.cpu()
        logger.info(f"finetune box branch: {ls.shape[0]} steps on {len(batch)} support images, (loc, ctr, iou) "
                    f"{[round(float(v), 4) for v in ls[0]]} -> {[round(float(v), 4) for v in ls[-1]]}")
        return branch

    @staticmethod
    def _finetune_codes(model, support_loader, class_codes, finetune: Dict[str, Any]):
        """The TFA step of one (dataset, seed): `class_codes` (None: the checkpoint's own cls_logits rows) refined on that seed's support
        images, every support record's boxes labelled with its item's support_set_target (the row of its code).  finetune: the keyword
        arguments of MetaOneStageDetector.finetune_class_codes (iters, lr, ..., batch_size: support images per network pass, default 16)."""
        if D.get_world_size() > 1:
            raise NotImplementedError(f"finetune: a rank sees its own shard of the support set and gradients are not reduced across ranks; "
                                      f"world size is {D.get_world_size()}")
        if support_loader is None:
            raise ValueError("finetune needs the support images: pass support_loader (or override the support-set loader builder)")
        kw = {k: v for k, v in finetune.items() if k != "box_branch"}
        kw.setdefault("batch_size", 16)
        batch = MetaFCOSRunner._support_batch(support_loader)
        codes, losses = model.finetune_class_codes(batch, class_codes, **kw)
        ls = losses.cpu()
        logger.info(f"finetune: {ls.numel()} steps on {len(batch)} support images, loss {float(ls[0]):.4f} -> {float(ls[-1]):.4f}")
        return codes

    def _episode(self, cfg, model, support_loader, query_loader, evaluator=None, base_support_loader=None,
                 output_folder: Optional[str] = None, num_classes: Optional[int] = None, eval_with_pretrained_code: bool = False,
                 finetune: Optional[Dict[str, Any]] = None):
        """ONE (dataset, seed) of meta_fcos_runner.py:497-560: support codes -> gather -> (base-class reduce + replace) ->
        normalise -> format -> [finetune: the codes refined on the support images] -> query loop.  Returns (evaluator results,
        formatted class codes)."""
        class_codes = None
        if not eval_with_pretrained_code:
            class_codes = self._episode_codes(cfg, model, support_loader, base_support_loader, output_folder, num_classes)
        installed = False
        try:
            if finetune is not None:
                class_codes = self._finetune_codes(model, support_loader, class_codes, finetune)
                eval_with_pretrained_code = False  # the refined rows are passed as class codes, also where they started as cls_logits
                if finetune.get("box_branch") is not None:
                    # the box branch trained on the same support images and installed for this seed's query loop only
                    branch = self._finetune_box_branch(model, support_loader, finetune["box_branch"])
                    model.set_box_branch(branch)
                    installed = True
            res = inference_on_dataset_with_class_codes(model, query_loader, evaluator, class_codes,
                                                        eval_with_pretrained_code=eval_with_pretrained_code)
        finally:
            if installed:
                model.set_box_branch(None)
        return res, class_codes

    def _do_test_meta_learning(self, cfg, model, support_loader=None, query_loader=None, evaluator=None, base_support_loader=None,
                               output_folder: Optional[str] = None, num_classes: Optional[int] = None, train_iter=None,
                               model_tag: str = "default", dataset_names: Optional[List[str]] = None, fuse_repeats: bool = False,
                               cache_queries: bool = False, cache_max_bytes: Optional[int] = None, shot_bank=None, bank_draws=None,
                               finetune: Optional[Dict[str, Any]] = None):
        """meta_fcos_runner.py:451-672.

        * With explicit loaders (support_loader + query_loader): ONE dataset / seed; returns (results, class_codes) -- the form
          the episode tests and bench use.
        * Without: the reference's full loop -- for seed in range(TEST.REPEAT_TEST if final else 1), for dataset in
          DATASETS.TEST (or `dataset_names`): loaders from the build_* methods (seeded support sets, :497-503),
          EVAL_WITH_PRETRAINED_CODE on "base" datasets (:483-486), USE_ALL_GTS_IN_BASE_CLASSES (:507-518), then
          results[f"seed{s}"][dataset] per run, results[model_tag][dataset] = the mean over seeds of every "bbox" metric
          (:589-603) plus AP / APr / APc / APf "_avg" and "_std" over the seeds (:604-620); returns the results dict.
        * fuse_repeats=True with REPEAT_TEST > 1: every seed's class codes are built first and the query set of a dataset runs ONCE
          against all of them (inference_on_dataset_with_code_sets: one backbone / tower pass per query batch, one evaluator per
          seed); the results dict is the one of the loop above.  EVAL_WITH_PRETRAINED_CODE datasets and multi-rank runs keep one query
          pass per seed.
        * cache_queries=True: ONE network pass per dataset's query set, kept as query records (evaluation.cache_query_dataset, at most
          cache_max_bytes of device memory; default: half of what is free); every seed is then scored from the records -- class-conditional
          conv and decode only.  A dataset whose records would not fit (estimated from its first record) keeps the plain loop, with a
          logged reason.  The results dict is the one of the loop above.
        * shot_bank=ShotBank with bank_draws=[(shots, seed), ...]: no support pass at all -- every draw's class codes come from the bank
          (evaluation.class_codes_from_bank on shot_bank.draw(shots, seed)); the query side runs as above, on query_loader, or on the
          datasets' loaders, or (cache_queries) on their records.  Returns results[f"shots{K}_seed{s}"][dataset] (dataset "query" for an
          explicit query_loader).  One rank only.
        * finetune=dict(iters=..., lr=..., ...): the TFA baseline -- every seed's class codes (on an EVAL_WITH_PRETRAINED_CODE dataset the
          checkpoint's cls_logits rows) are refined on that seed's support images before its query loop (_finetune_codes;
          sylph_amd.finetune).  One rank only; not together with fuse_repeats or a shot bank.
          finetune=dict(..., box_branch=dict(iters=..., lr=..., ...)) also trains the box branch on the same support images (the
          Meta-FCOS-pretrain-tfa-finetune yamls leave FREEZE_BBOX_BRANCH off) and installs it for that seed's query loop, restoring
          the checkpoint's in a `finally`; not together with cache_queries, fuse_repeats or a shot bank."""
        if finetune is not None:
            if D.get_world_size() > 1:
                raise NotImplementedError(f"finetune: a rank sees its own shard of the support set and gradients are not reduced across ranks; "
                                          f"world size is {D.get_world_size()}")
            if shot_bank is not None or bank_draws is not None or fuse_repeats:
                raise NotImplementedError("finetune together with fuse_repeats or a shot bank is not supported: the codes of every seed are "
                                          "refined on that seed's support images, one query pass per seed")
            if finetune.get("box_branch") is not None:
                for on, what in ((cache_queries, "cache_queries"), (fuse_repeats, "fuse_repeats"), (shot_bank is not None or bank_draws is not None, "a shot bank")):
                    if on:
                        raise NotImplementedError(f"finetune box_branch together with {what} is not supported: the query records / fused passes "
                                                  f"were made under another box branch than the one each seed trains")
        if shot_bank is not None or bank_draws is not None:
            return self._bank_sweep(cfg, model, shot_bank, bank_draws, query_loader, evaluator, dataset_names, cache_queries, cache_max_bytes)
        if support_loader is not None or query_loader is not None:
            return self._episode(cfg, model, support_loader, query_loader, evaluator, base_support_loader, output_folder, num_classes,
                                 finetune=finetune)
        names = list(dataset_names if dataset_names is not None else cfg.DATASETS.TEST)
        assert len(names)
        max_iter = cfg.get("SOLVER", {}).get("MAX_ITER", None) if hasattr(cfg, "get") else None
        is_final = train_iter is None or (max_iter is not None and train_iter == max_iter - 1)
        repeat = int(cfg.TEST.REPEAT_TEST) if is_final and "TEST" in cfg and "REPEAT_TEST" in cfg.TEST else 1
        if is_final and "TEST" in cfg and bool(cfg.TEST.get("AUG", {}).get("ENABLED", False)):
            # meta_fcos_runner.py:633-651 wraps the model in GeneralizedRCNNWithTTA here, which a MetaOneStageDetector cannot go through.
            # This model runs the views itself (forward_instances_views reads cfg.TEST.AUG): the ordinary query loop below IS the
            # test-time-augmented evaluation; the query loader must hand out the uint8 originals ("image_u8")
            logger.info("Running inference with test-time augmentation ...")
        results = OrderedDict()
        results[model_tag] = OrderedDict()
        main = D.get_rank() == 0

        def is_pretrained(name):
            return "base" in name and bool(cfg.MODEL.META_LEARN.EVAL_WITH_PRETRAINED_CODE)

        def folder_of(name, seed):
            if output_folder or cfg.get("OUTPUT_DIR", None):
                return os.path.join(output_folder or cfg.OUTPUT_DIR, "inference", model_tag,
                                    str(train_iter) if train_iter is not None else "final", name, str(seed))
            return None

        def support_loaders(name, seed):
            sup = self.build_episodic_learning_detection_test_support_set_loader(cfg, name, seed)
            base = None
            if bool(cfg.MODEL.META_LEARN.USE_ALL_GTS_IN_BASE_CLASSES):
                base = self.build_episodic_learning_detection_test_support_set_base_loader(cfg, name)
            return sup, base

        fused = {}  # (seed, dataset) -> evaluator results of the one fused query pass of that dataset
        if fuse_repeats and repeat > 1:
            if D.get_world_size() > 1:
                logger.info("fuse_repeats: a multi-rank run keeps one query pass per seed (every pass ends in its evaluator's own gather)")
            else:
                for name in names:
                    if is_pretrained(name):
                        continue  # no class codes to vary: the unfused loop below
                    sets, evs = [], []
                    for seed in range(repeat):
                        sup, base = support_loaders(name, seed)
                        sets.append(self._episode_codes(cfg, model, sup, base, folder_of(name, seed), self._global_len(sup)))
                        evs.append(self.get_evaluator(cfg, name, output_folder=folder_of(name, seed)))
                    qry = self.build_episodic_learning_detection_test_query_loader(cfg, name)
                    for seed, per in enumerate(inference_on_dataset_with_code_sets(model, qry, evs, sets)):
                        fused[(seed, name)] = per
        cached = {}  # dataset -> its query records, in loader order
        if cache_queries:
            for name in names:
                if any((seed, name) not in fused for seed in range(repeat)):
                    try:
                        cached[name] = cache_query_dataset(model, self.build_episodic_learning_detection_test_query_loader(cfg, name),
                                                           max_bytes=cache_max_bytes)
                    except MemoryError as e:
                        logger.info(f"cache_queries: {name} keeps one network pass per seed ({e})")
        for seed in range(repeat):
            logger.info(f"{seed} out of {repeat} tests.")
            results[f"seed{seed}"] = OrderedDict()
            for name in names:
                pretrained = is_pretrained(name)
                if (seed, name) in fused:
                    per = fused[(seed, name)]
                else:
                    folder = folder_of(name, seed)
                    sup = base = None
                    if not pretrained or finetune is not None:
                        sup, base = support_loaders(name, seed)
                    qry = cached[name] if name in cached else self.build_episodic_learning_detection_test_query_loader(cfg, name)
                    ev = self.get_evaluator(cfg, name, output_folder=folder)
                    n_cls = self._global_len(sup) if sup is not None else None
                    per, _ = self._episode(cfg, model, sup, qry, ev, base, folder, n_cls, eval_with_pretrained_code=pretrained, finetune=finetune)
                if not main:
                    continue
                results[f"seed{seed}"][name] = per
                bbox = per.get("bbox") if isinstance(per, dict) else None
                if seed == 0:
                    results[model_tag][name] = {k: (dict(v) if isinstance(v, dict) else v) for k, v in per.items()} \
                        if isinstance(per, dict) else per
                elif bbox is not None:
                    acc = results[model_tag][name]["bbox"]
                    for k in acc:
                        acc[k] += bbox[k]
                        if seed == repeat - 1:
                            acc[k] /= repeat
                if is_final and seed == repeat - 1 and bbox is not None:
                    import numpy as np
                    for k in ("AP", "APr", "APc", "APf"):
                        hist = [results[f"seed{s}"][name]["bbox"][k] for s in range(repeat) if k in results[f"seed{s}"][name]["bbox"]]
                        if hist:
                            results[model_tag][name]["bbox"][f"{k}_avg"] = float(np.array(hist).mean())
                            results[model_tag][name]["bbox"][f"{k}_std"] = float(np.array(hist).std())
        for recs in cached.values():
            release_query_records(recs)
        return results

    def _bank_sweep(self, cfg, model, shot_bank, bank_draws, query_loader=None, evaluator=None, dataset_names=None,
                    cache_queries: bool = False, cache_max_bytes: Optional[int] = None):
        """_do_test_meta_learning with a shot bank: one query evaluation per (shots, seed) draw, class codes from the bank."""
        world = D.get_world_size()
        if world > 1:
            raise NotImplementedError(f"shot_bank: a bank's rows live on one device and its draws are not gathered across ranks; world size is "
                                      f"{world}, run the sweep on one rank")
        if shot_bank is None or not bank_draws:
            raise ValueError("shot_bank and bank_draws go together: a ShotBank and a non-empty list of (shots, seed) draws")
        if query_loader is not None:
            datasets = [("query", query_loader, evaluator)]
        else:
            names = list(dataset_names if dataset_names is not None else cfg.DATASETS.TEST)
            assert len(names)
            datasets = [(name, None, None) for name in names]
        results = OrderedDict()
        cached = {}
        try:
            for shots, seed in bank_draws:
                idx, seg_len, class_ids = shot_bank.draw(int(shots), int(seed))
                codes = class_codes_from_bank(model, shot_bank, idx, seg_len, class_ids)
                class_codes = format_class_codes_shared(codes, device=model.device)
                tag = f"shots{int(shots)}_seed{int(seed)}"
                results[tag] = OrderedDict()
                for name, loader, ev in datasets:
                    if loader is None:
                        ev = self.get_evaluator(cfg, name)
                        if name not in cached and cache_queries:
                            try:
                                cached[name] = cache_query_dataset(model, self.build_episodic_learning_detection_test_query_loader(cfg, name),
                                                                   max_bytes=cache_max_bytes)
                            except MemoryError as e:
                                cached[name] = None
                                logger.info(f"cache_queries: {name} keeps one network pass per draw ({e})")
                        loader = cached.get(name) or self.build_episodic_learning_detection_test_query_loader(cfg, name)
                    results[tag][name] = inference_on_dataset_with_class_codes(model, loader, ev, class_codes)
        finally:
            for recs in cached.values():
                if recs:
                    release_query_records(recs)
        return results

    def do_test(self, cfg, model, train_iter=None, support_loader=None, query_loader=None, evaluator=None):
        """meta_fcos_runner.py:674-701.  With explicit episodic loaders: one episode (sylph_amd.data has synthetic ones emitting
        the reference's item shapes).  Without: the multi-seed / multi-dataset loop over the build_* loader methods."""
        if not cfg.MODEL.META_LEARN.EPISODIC_LEARNING:
            raise NotImplementedError("base-detector evaluation is out of scope")
        if support_loader is None and query_loader is None:
            return self._do_test_meta_learning(cfg, model, train_iter=train_iter)
        if support_loader is None or query_loader is None:
            raise NotImplementedError(
                "dataset registration/loading (sylph/data/*) is out of scope: pass support_loader and query_loader")
        res, _ = self._do_test_meta_learning(cfg, model, support_loader, query_loader, evaluator)
        return OrderedDict(default=res)


class MetaFCOSROIEncoderRunner(MetaFCOSRunner):
    """sylph/runner/meta_fcos_roi_encoder_runner.py: ROIEncoder config defaults."""

    def get_default_cfg(self):
        return _config.get_roi_encoder_default_cfg()
