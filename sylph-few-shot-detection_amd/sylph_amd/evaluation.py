"""Episodic inference loops and class-code formatting with the reference's signatures
(sylph/evaluation/meta_learn_evaluation.py:71-470).  The loops are host control flow only; the
model they drive enqueues HIP kernels.  Timing/log lines follow the reference protocol (warm-up
iterations excluded, "s / img", "s / class code")."""
import logging
import os
import time
from contextlib import ExitStack, contextmanager
from typing import Any, Dict, List

import torch
from torch import nn

from .distributed import get_world_size

logger = logging.getLogger(__name__)


@contextmanager
def inference_context(model: nn.Module):
    """detectron2.evaluation.inference_context: temporarily eval()."""
    mode = model.training
    model.eval()
    try:
        yield
    finally:
        model.train(mode)


def format_class_codes_shared(class_codes: List[Dict[str, Any]], device) -> Dict[str, torch.Tensor]:
    """The per-class records of loop A as one tensor per code field, row c = the class whose support_set_target is c
    (semantics of meta_learn_evaluation.py:71-103: fields other than "snnl", cls_bias flattened to (n,); an empty list is
    returned as it is; a class id nobody delivered fails in torch.cat like the reference's None slot does)."""
    n = len(class_codes)
    if n == 0:
        return class_codes
    fields = [f for f in class_codes[0]["class_code"] if f != "snnl"]
    by_target = {int(rec["support_set_target"]): rec["class_code"] for rec in class_codes}
    packed = {}
    for f in fields:
        rows = [by_target[c][f].to(device) if c in by_target and f in by_target[c] else None for c in range(n)]
        t = torch.cat(rows, dim=0)
        packed[f] = t.reshape(-1) if f == "cls_bias" else t
    if "snnl" in class_codes[0]["class_code"]:  # the reference keeps the key with its initial None slots and fails on it in cat
        raise TypeError("expected Tensor as element 0 in argument 0, but got NoneType")
    return packed


def inference_normalization(model, codes: List[Dict[str, Any]]):
    """meta_learn_evaluation.py:105-116: the run_type "meta_learn_normalize_code" call under eval mode and no_grad."""
    logger.info(f"Start normalizing class codes on {get_world_size()} devices")
    was_training = isinstance(model, nn.Module) and model.training
    if isinstance(model, nn.Module):
        model.eval()
    try:
        with torch.no_grad():
            return model(batched_inputs=None, class_code=codes, run_type="meta_learn_normalize_code")
    finally:
        if was_training:
            model.train(True)


def class_padded_hw(support_set, divisibility: int = 32):
    """(H, W) one class's support images are padded to when the class runs alone (ImageList.from_tensors: the maximum over its
    images, rounded up to the backbone's size divisibility)."""
    d = int(divisibility)
    if len(support_set) == 0:
        return (0, 0)
    h = max(int(rec["image"].shape[-2]) for rec in support_set)
    w = max(int(rec["image"].shape[-1]) for rec in support_set)
    return ((h + d - 1) // d * d, (w + d - 1) // d * d)


def _log_totals(kind: str, unit: str, total_time: float, compute_time: float, n: int, devices: int):
    logger.info("Total inference time: {:.3f}s ({:.6f} s / {} per device, on {} devices)".format(
        total_time, total_time / max(n, 1), unit, devices))
    logger.info("Total inference pure compute time: {:.3f}s ({:.6f} s / img per device, on {} devices)".format(
        compute_time, compute_time / max(n, 1), devices))


def inference_on_support_set_dataset(model, data_loader, output_dir: str = None) -> List[Dict[str, Any]]:
    """Loop A (meta_learn_evaluation.py:256-365): one item = one class {"support_set", "support_set_target",
    "class_name"}; returns [{support_set_target, class_name, class_code}] and optionally writes
    <output_dir>/<class_name>.pth (the file SylphPredictor reads, sylph/predictor.py:167-187)."""
    devices = get_world_size()
    total = len(data_loader)
    logger.info(f"Start generating class codes on {total} support sets on {devices} devices")
    if output_dir is not None:
        os.makedirs(output_dir, exist_ok=True)
    num_warmup = min(5, max(total - 1, 0))
    start_time, compute = time.perf_counter(), 0.0
    results = []
    with ExitStack() as stack:
        if isinstance(model, nn.Module):
            stack.enter_context(inference_context(model))
        stack.enter_context(torch.no_grad())
        # Classes are grouped into batches of up to SYLPH_SUPPORT_BATCH support images (default 64) that share the backbone and
        # code-generator launches (model.forward_class_codes); the loader still yields -- and the model API still accepts --
        # one class per item, as in the reference.  Only classes with the same shot count AND the same padded size (see
        # class_padded_hw) share a batch, so every class sees exactly the tensors of its own one-class call.
        # SYLPH_SUPPORT_BATCH=0: one call per class.
        cap = int(os.environ.get("SYLPH_SUPPORT_BATCH", "64"))
        batched = cap > 0 and hasattr(model, "forward_class_codes")
        group: List[Any] = []

        def flush():
            nonlocal compute
            if not group:
                return
            t0 = time.perf_counter()
            if batched and len(group) > 1:
                codes = model.forward_class_codes([g for g in group])
            else:
                codes = [model(g, run_type="meta_learn_test_support") for g in group]
            codes = [{k: (v.cpu() if torch.is_tensor(v) else v) for k, v in c.items()} for c in codes]  # device sync
            compute += time.perf_counter() - t0
            for g, c in zip(group, codes):
                result = {k: v for k, v in g[0].items() if k != "support_set"}
                result["class_code"] = c
                if output_dir is not None:
                    torch.save(result, os.path.join(output_dir, f"{result['class_name']}.pth"))
                results.append(result)
            group.clear()

        n_img = 0
        for idx, inputs in enumerate(data_loader):
            assert len(inputs) == 1, "inputs' batch size is not 1"
            if idx == num_warmup:
                flush()
                n_img = 0
                start_time, compute = time.perf_counter(), 0.0
            k = len(inputs[0]["support_set"])
            # A class may only join a group whose padded batch size equals the size the class would be padded to ALONE (the max
            # over ALL of its support images, rounded up to the size divisibility): the reference pads one class per call
            # (meta_one_stage_detector.py:229-254), and the activations next to the right / bottom border depend on that size.
            same = not group or (len(group[0][0]["support_set"]) == k and
                                 class_padded_hw(group[0][0]["support_set"]) == class_padded_hw(inputs[0]["support_set"]))
            if group and (not batched or not same or n_img + k > cap):
                flush()
                n_img = 0
            group.append(inputs)
            n_img += k
        flush()
    _log_totals("support", "class code", time.perf_counter() - start_time, compute, total - num_warmup, devices)
    return results


def inference_on_support_set_dataset_base(model, data_loader, all_id_map=None, base_id_map=None,
                                          output_dir: str = None) -> List[Dict[str, Any]]:
    """Base-class variant (meta_learn_evaluation.py:118-254): a class arrives in chunks of <= 10 shots
    carrying "len"/"total_len"; chunk codes are accumulated with weight len/total_len and the
    accumulated weight is kept in "acc_weight" for the cross-rank reduce."""
    from . import distributed as D
    rows, names, engine = [], {}, getattr(model, "engine", None)
    with ExitStack() as stack:
        if isinstance(model, nn.Module):
            stack.enter_context(inference_context(model))
        stack.enter_context(torch.no_grad())
        for inputs in data_loader:
            assert len(inputs) == 1, "inputs' batch size is not 1"
            code = model(inputs, run_type="meta_learn_test_support")  # device tensors; nothing is read back per chunk
            cid = int(inputs[0]["support_set_target"])
            names[cid] = inputs[0]["class_name"]
            weight = float(inputs[0]["len"]) / inputs[0]["total_len"]
            wn = code["cls_weight_norm"].reshape(1) * weight if "cls_weight_norm" in code else None
            D.require_1x1_codes(code["cls_conv"], "inference_on_support_set_dataset_base (chunk accumulation)")
            rows.append(D.pack_codes(code["cls_conv"].reshape(1, 256) * weight, code["cls_bias"].reshape(1) * weight, [cid],
                                     [weight], wn, [names[cid]]))
    if not rows:
        return []
    packed = torch.cat(rows).contiguous()
    ncls = max(names) + 1
    # per-class accumulation of the weighted chunk codes in arrival order: ONE segmented reduce on the device
    # (sylph_reduce_codes, divide_by_acc = 0); acc_weight keeps the accumulated weight for the cross-rank reduce
    if engine is not None and packed.is_cuda:
        red = engine.reduce_codes(packed, ncls, divide_by_acc=False)
    else:
        red = D.scatter_by_class_id(D.reduce_packed_codes(packed, divide_by_acc=False), ncls)
    red = red.cpu()  # the only read-back of the loop
    results = []
    for cid in names:  # first-appearance order, as the reference's dict
        r = red[cid]
        cc = {"cls_conv": r[:256].reshape(1, 256, 1, 1).clone(), "cls_bias": r[256:257].reshape(1, 1, 1, 1).clone(),
              "acc_weight": float(r[D.F_ACC])}
        if float(r[D.F_HAS_WNORM]) > 0:
            cc["cls_weight_norm"] = r[D.F_WNORM:D.F_WNORM + 1].reshape(1, 1, 1, 1).clone()
        results.append({"support_set_target": cid, "class_name": names[cid], "class_code": cc})
    return results


def plan_roi_segments(records: List[Dict[str, Any]], chunk: int = 10):
    """Annotated records -> the ROI list of ONE batch that holds each image once.  Every instance (instances.gt_boxes[i] with
    instances.gt_classes[i]) is a support shot of its class; the shots of a class follow image order, then box order, and are cut
    into segments of at most `chunk` shots (the chunking of the base-class path, meta_learn_evaluation.py:118-254); the segments
    of a class are consecutive and the classes come in order of first appearance.  A record without boxes contributes nothing.
    Returns (boxes (R, 4) fp32, roi_image [R], seg_len [n_seg], seg_class [n_seg]).  Pure host code, no random choice."""
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"chunk must be at least 1, got {chunk}")
    shots: Dict[int, List[Any]] = {}  # class id -> [(image, box)], dicts keep first-appearance order
    for b, rec in enumerate(records):
        inst = rec.get("instances") if isinstance(rec, dict) else None
        if inst is None or len(inst.gt_boxes.tensor) == 0:
            continue
        gt = inst.gt_boxes.tensor.detach().float().cpu().reshape(-1, 4)
        cls = torch.as_tensor(inst.gt_classes).reshape(-1).tolist()
        assert len(cls) == gt.shape[0], f"record {b}: {len(cls)} classes for {gt.shape[0]} boxes"
        for i, cid in enumerate(cls):
            shots.setdefault(int(cid), []).append((b, gt[i]))
    boxes, roi_image, seg_len, seg_class = [], [], [], []
    for cid, items in shots.items():
        for k in range(0, len(items), chunk):
            part = items[k:k + chunk]
            boxes.extend(bx for _, bx in part)
            roi_image.extend(b for b, _ in part)
            seg_len.append(len(part))
            seg_class.append(cid)
    return (torch.stack(boxes) if boxes else torch.zeros(0, 4)), roi_image, seg_len, seg_class


def inference_on_annotated_images(model, data_loader, chunk: int = 10, class_names=None, output_dir: str = None) -> List[Dict[str, Any]]:
    """Base-class codes from annotated images at one backbone pass per image.  Each loader item is a list of annotated records
    ("image", "instances" with gt_boxes / gt_classes); plan_roi_segments turns the item into one ROI list and
    model.forward_class_codes_rois runs it as ONE batch.  Every segment code is weighted by its instance count and the rows of
    the whole loader are reduced once on the device (Engine.reduce_codes, divide_by_acc): a class's code is the
    instance-count-weighted mean of its chunk codes, the len / total_len weighting of inference_on_support_set_dataset_base.
    Returns that function's records (first-appearance class order), so normalisation, the cross-rank gather and the .pth files
    SylphPredictor reads work unchanged.  `class_names`: class id -> name (a dict or a sequence); default str(id)."""
    from . import distributed as D
    engine = getattr(model, "engine", None)
    if output_dir is not None:
        os.makedirs(output_dir, exist_ok=True)

    def name_of(cid: int) -> str:
        if class_names is None:
            return str(cid)
        return str(class_names[cid])

    rows, names = [], {}
    with ExitStack() as stack:
        if isinstance(model, nn.Module):
            stack.enter_context(inference_context(model))
        stack.enter_context(torch.no_grad())
        for records in data_loader:
            boxes, roi_image, seg_len, seg_class = plan_roi_segments(records, chunk)
            if not seg_len:
                continue
            segments, r0 = [], 0
            for n in seg_len:
                segments.append({"image_index": torch.tensor(roi_image[r0:r0 + n], dtype=torch.long), "boxes": boxes[r0:r0 + n]})
                r0 += n
            codes = model.forward_class_codes_rois(records, segments)  # device tensors; nothing is read back per item
            for cid in seg_class:
                names.setdefault(cid, name_of(cid))
            w = torch.tensor(seg_len, dtype=torch.float32, device=codes[0]["cls_conv"].device)
            D.require_1x1_codes(codes[0]["cls_conv"], "inference_on_annotated_images (chunk accumulation)")
            conv = torch.cat([c["cls_conv"].reshape(1, 256) for c in codes]) * w[:, None]
            bias = torch.cat([c["cls_bias"].reshape(1) for c in codes]) * w
            wn = torch.cat([c["cls_weight_norm"].reshape(1) for c in codes]) * w if "cls_weight_norm" in codes[0] else None
            rows.append(D.pack_codes(conv, bias, seg_class, seg_len, wn, [names[cid] for cid in seg_class]))
    if not rows:
        return []
    packed = torch.cat(rows).contiguous()
    ncls = max(names) + 1
    if engine is not None and packed.is_cuda:
        red = engine.reduce_codes(packed, ncls, divide_by_acc=True)
    else:
        red = D.scatter_by_class_id(D.reduce_packed_codes(packed, divide_by_acc=True), ncls)
    red = red.cpu()  # the only read-back of the loop
    results = []
    for cid in names:  # first-appearance order
        r = red[cid]
        cc = {"cls_conv": r[:256].reshape(1, 256, 1, 1).clone(), "cls_bias": r[256:257].reshape(1, 1, 1, 1).clone(),
              "acc_weight": float(r[D.F_ACC])}
        if float(r[D.F_HAS_WNORM]) > 0:
            cc["cls_weight_norm"] = r[D.F_WNORM:D.F_WNORM + 1].reshape(1, 1, 1, 1).clone()
        result = {"support_set_target": cid, "class_name": names[cid], "class_code": cc}
        if output_dir is not None:
            torch.save(result, os.path.join(output_dir, f"{result['class_name']}.pth"))
        results.append(result)
    return results


def build_shot_bank(model, data_loader, chunk: int = 10):
    """A ShotBank of every annotated instance of a loader, at one backbone pass per image.  The loader is
    inference_on_annotated_images': each item a list of annotated records, run as ONE batch (model.forward_shot_rows).  A row is
    remembered with its class id, its image id (the record's "image_id", else the running image count) and its annotation index
    within the record.  `chunk` is inference_on_annotated_images' argument, accepted so that the two take the same call; a bank
    row is per instance and does not depend on it (segments are cut at the draw)."""
    from .shots import ShotBank
    if int(chunk) < 1:
        raise ValueError(f"chunk must be at least 1, got {chunk}")
    engine = model.engine
    bank = ShotBank(engine.shot_key(), device=engine.device)
    bank.stamp = engine.codegen_stamp()
    seen = 0
    with ExitStack() as stack:
        if isinstance(model, nn.Module):
            stack.enter_context(inference_context(model))
        stack.enter_context(torch.no_grad())
        for records in data_loader:
            rows, image_index, ann_index, class_ids = model.forward_shot_rows(records)
            if rows is not None:
                ids = [int(rec.get("image_id", seen + b)) for b, rec in enumerate(records)]
                bank.append(rows, class_ids, [ids[b] for b in image_index], ann_index)
            seen += len(records)
    bank.tensor()
    logger.info(f"Banked {len(bank)} support instances of {len(bank.classes())} classes from {seen} images, {bank.nbytes} device bytes")
    return bank


def build_roi_bank(model, data_loader):
    """A RoiBank (sylph_amd.metatrain) of every annotated instance of a loader, at one backbone pass per image: the 7x7x256 ROI maps the
    code generator's training forward starts from.  The loader is build_shot_bank's: each item a list of annotated records, run as ONE
    batch (model.forward_roi_rows).  The rows depend on the backbone alone, not on the generator."""
    from .metatrain import RoiBank
    engine = model.engine
    bank = RoiBank(device=engine.device)
    seen = 0
    with ExitStack() as stack:
        if isinstance(model, nn.Module):
            stack.enter_context(inference_context(model))
        stack.enter_context(torch.no_grad())
        for records in data_loader:
            rows, class_ids = model.forward_roi_rows(records)
            if rows is not None:
                bank.append(rows, class_ids)
            seen += len(records)
    bank.tensor()
    logger.info(f"Banked {len(bank)} ROI maps of {len(bank.classes())} classes from {seen} images, {bank.nbytes} device bytes")
    return bank


def class_codes_from_bank(model, bank, idx, seg_len, class_ids, class_names=None, normalize: bool = True) -> List[Dict[str, Any]]:
    """The class codes of one draw from a ShotBank (bank.draw), with no support pass: segment j -- the rows idx[...] of seg_len[j]
    shots -- is class class_ids[j].  Returns inference_on_annotated_images' records ({"support_set_target", "class_name",
    "class_code": {"cls_conv" (1, 256, k, k), "cls_bias" (1, 1, 1, 1)[, "cls_weight_norm" (1, 1, 1, 1)]}}, host tensors; no
    "acc_weight": a draw's code is whole, nothing is left to accumulate) in the order of the segments; the codes are bit for bit those of model.forward_class_codes_rois on segments holding
    the same instances in the same order (Engine.combine_shots).  normalize: the records then go through inference_normalization
    (sylph_normalize_codes with cls_weight_norm) like the runner's; the ROIEncoder's codes need none."""
    engine = model.engine
    bank.check_key(engine)
    bank.check_stamp(engine)
    if len(class_ids) != len(seg_len):
        raise ValueError(f"{len(class_ids)} class ids for {len(seg_len)} segments")
    with torch.no_grad():
        codes, wn = engine.combine_shots(bank.tensor(), idx, seg_len)
    codes = codes.cpu()  # the only read-back of the draw
    wn = wn.cpu() if wn is not None else None
    k, n = engine.code_ksize, 256 * engine.code_ksize ** 2
    results = []
    for j, cid in enumerate(class_ids):
        cc = {"cls_conv": codes[j, :n].reshape(1, 256, k, k).clone(), "cls_bias": codes[j, n:n + 1].reshape(1, 1, 1, 1).clone()}
        if wn is not None:
            cc["cls_weight_norm"] = wn[j:j + 1].reshape(1, 1, 1, 1).clone()
        name = str(cid) if class_names is None else str(class_names[cid])
        results.append({"support_set_target": int(cid), "class_name": name, "class_code": cc})
    if normalize and not engine.is_roi_encoder:
        results = inference_normalization(model, results)
    return results


class _NoOpEvaluator:
    def reset(self):
        pass

    def process(self, inputs, outputs):
        pass

    def evaluate(self):
        return {}


def _evaluator_inputs(inputs):
    """what evaluator.process is shown for a query batch: the batch itself, or the stored metadata of a record-input (cache_query_dataset)"""
    if isinstance(inputs, (list, tuple)) and len(inputs) == 1 and isinstance(inputs[0], dict) and "record" in inputs[0]:
        return inputs[0]["inputs"]
    return inputs


def release_query_records(records):
    """close every QueryRecord of a cache_query_dataset list (their device bytes go back to the engine)"""
    for item in records:
        for x in item:
            if isinstance(x, dict) and hasattr(x.get("record"), "close"):
                x["record"].close()


def cache_query_dataset(model, data_loader, max_bytes=None) -> List[Any]:
    """ONE network pass over a query loader, no class codes: model(inputs, run_type="meta_learn_cache_query") per batch -> the list of
    what it returned, in loader order: per batch a list of one record-input ({"record": QueryRecord, "inputs": metadata per image}; no
    image tensors are kept).  inference_on_dataset_with_class_codes and inference_on_dataset_with_code_sets take the list in place of the
    loader, any number of times: every seed or shot setting of the reference's protocol (meta_fcos_runner.py:451-672 over
    meta_learn_evaluation.py:367-470) is then scored without the backbone and the towers.
    max_bytes: device bytes the records may hold (default: half of the free device memory at the call).  MemoryError, naming the bytes
    needed and allowed, BEFORE the store that would pass it: as soon as the first record shows that the whole loader would (its bytes x
    the loader's length), or when the records so far plus one more batch at the bytes per image seen so far would.  Nothing stays allocated
    then.  release_query_records(list) gives the bytes back when the list is no longer needed."""
    if max_bytes is None and torch.cuda.is_available():
        max_bytes = int(torch.cuda.mem_get_info()[0]) // 2
    try:
        total = len(data_loader)
    except TypeError:
        total = None
    records: List[Any] = []
    used, images = 0, 0

    def refuse(needed: int, why: str):
        release_query_records(records)
        raise MemoryError(f"cache_query_dataset: {why} needs {needed} bytes of query records, {max_bytes} are allowed (max_bytes); "
                          "nothing is kept")

    with ExitStack() as stack:
        if isinstance(model, nn.Module):
            stack.enter_context(inference_context(model))
        stack.enter_context(torch.no_grad())
        for idx, inputs in enumerate(data_loader):
            if max_bytes is not None and images:
                nxt = used + (used * len(inputs) + images - 1) // images
                if nxt > max_bytes:
                    refuse(nxt, f"batch {idx} on top of the {len(records)} stored")
            out = model(inputs, run_type="meta_learn_cache_query")
            records.append(out)
            used += int(out[0]["record"].nbytes)
            images += len(inputs)
            if max_bytes is not None:
                if idx == 0 and total is not None and used * total > max_bytes:
                    refuse(used * total, f"the whole loader ({total} batches of about {used} bytes each)")
                if used > max_bytes:
                    refuse(used, f"batch {idx}")
    logger.info(f"Cached {images} query images as {len(records)} records, {used} device bytes")
    return records


def inference_on_dataset_with_class_codes(model, data_loader, evaluator, class_codes, cls_reweight=False,
                                          eval_with_pretrained_code=False):
    """Loop B (meta_learn_evaluation.py:367-470): model(inputs, class_code=..., run_type=
    "meta_learn_test_instance") per query batch, evaluator.process(inputs, outputs), evaluator.evaluate().
    data_loader may be the list cache_query_dataset returned: the model then scores the stored records, and evaluator.process receives
    the stored metadata of each batch as `inputs`."""
    devices = get_world_size()
    if eval_with_pretrained_code:
        assert class_codes is None  # meta_learn_evaluation.py:376-378: the model's own cls_logits are the codes
    else:
        assert class_codes is not None
    if cls_reweight:
        raise NotImplementedError("cls_reweight is not supported (CLS_REWEIGHT is False in every yaml)")
    total = len(data_loader)
    logger.info(f"Start inference with {'pretrained' if eval_with_pretrained_code else 'predicted'} class codes on {total} images")
    evaluator = evaluator if evaluator is not None else _NoOpEvaluator()
    evaluator.reset()
    num_warmup = min(5, max(total - 1, 0))
    start_time, compute = time.perf_counter(), 0.0
    with ExitStack() as stack:
        if isinstance(model, nn.Module):
            stack.enter_context(inference_context(model))
        stack.enter_context(torch.no_grad())
        for idx, inputs in enumerate(data_loader):
            if idx == num_warmup:
                start_time, compute = time.perf_counter(), 0.0
            t0 = time.perf_counter()
            outputs = model(inputs, class_code=class_codes, run_type="meta_learn_test_instance")
            # forward_instances ends on the count read-back: the device work of this batch is complete
            compute += time.perf_counter() - t0
            evaluator.process(_evaluator_inputs(inputs), outputs)
    _log_totals("query", "img", time.perf_counter() - start_time, compute, total - num_warmup, devices)
    results = evaluator.evaluate()
    return results if results is not None else {}


def inference_on_dataset_with_code_sets(model, data_loader, evaluators, class_code_sets):
    """Loop B once for SEVERAL code sets: one pass over the query loader, model(inputs, class_code_sets=..., run_type=
    "meta_learn_test_instance") per batch (the backbone and towers run once, the class-conditional conv and decode per set); evaluator g
    sees what inference_on_dataset_with_class_codes would have shown it with class_code_sets[g] -> [evaluator_g.evaluate() for g].
    The reference runs the query set once per support seed (meta_fcos_runner.py:451-672 over meta_learn_evaluation.py:367-470).
    data_loader may be the list cache_query_dataset returned (see inference_on_dataset_with_class_codes)."""
    devices = get_world_size()
    class_code_sets = list(class_code_sets)
    if len(class_code_sets) == 0:
        raise ValueError("class_code_sets is empty")
    evaluators = [e if e is not None else _NoOpEvaluator() for e in (evaluators if evaluators is not None else [None] * len(class_code_sets))]
    if len(evaluators) != len(class_code_sets):
        raise ValueError(f"{len(evaluators)} evaluators for {len(class_code_sets)} code sets: one evaluator per set")
    total = len(data_loader)
    logger.info(f"Start inference with {len(class_code_sets)} sets of predicted class codes on {total} images")
    for e in evaluators:
        e.reset()
    num_warmup = min(5, max(total - 1, 0))
    start_time, compute = time.perf_counter(), 0.0
    with ExitStack() as stack:
        if isinstance(model, nn.Module):
            stack.enter_context(inference_context(model))
        stack.enter_context(torch.no_grad())
        for idx, inputs in enumerate(data_loader):
            if idx == num_warmup:
                start_time, compute = time.perf_counter(), 0.0
            t0 = time.perf_counter()
            outputs = model(inputs, class_code_sets=class_code_sets, run_type="meta_learn_test_instance")
            compute += time.perf_counter() - t0
            for e, out in zip(evaluators, outputs):
                e.process(_evaluator_inputs(inputs), out)
    _log_totals("query", "img", time.perf_counter() - start_time, compute, total - num_warmup, devices)
    results = [e.evaluate() for e in evaluators]
    return [r if r is not None else {} for r in results]


DET_ROW = 8  # image id | x0 | y0 | x1 | y1 | score | contiguous class id | valid


def detections_to_tensor(outputs: List[Dict[str, Any]], image_ids: List[int]) -> torch.Tensor:
    """Result sink, device side: every detection of a batch as one dense (n, 8) fp32 tensor on the device
    (image id, XYXY box, score, class, valid) -- no per-image / per-field .cpu() as in the d2 evaluators the reference
    calls from meta_learn_evaluation.py:428,465.  Image ids must be < 2^24 (exact in fp32)."""
    assert len(outputs) == len(image_ids)
    insts = [o["instances"] for o in outputs]
    dev = insts[0].pred_boxes.tensor.device if insts else torch.device("cpu")
    parts = []
    for img_id, i in zip(image_ids, insts):
        n = len(i)
        if n == 0:
            continue
        assert 0 <= int(img_id) < (1 << 24)
        parts.append(torch.cat([torch.full((n, 1), float(img_id), device=dev), i.pred_boxes.tensor.float(),
                                i.scores.float().unsqueeze(1), i.pred_classes.float().unsqueeze(1),
                                torch.ones(n, 1, device=dev)], dim=1))
    return torch.cat(parts) if parts else torch.zeros(0, DET_ROW, device=dev)


def gather_detection_rows(local: torch.Tensor, capacity: int) -> torch.Tensor:
    """Prediction gather across ranks (the reference pickles lists through comm.gather inside the evaluators): ONE
    all_gather_into_tensor of equal-size (capacity, 8) blocks, rank order preserved; rows with valid = 0 are padding.
    capacity >= the largest per-rank detection count (e.g. images per rank x POST_NMS_TOPK_TEST + ties)."""
    import torch.distributed as dist
    assert local.shape[0] <= capacity, f"{local.shape[0]} detections do not fit the gather block of {capacity}"
    block = torch.zeros(capacity, DET_ROW, dtype=torch.float32, device=local.device)
    block[: local.shape[0]] = local
    if not (dist.is_available() and dist.is_initialized()):
        return block
    out = torch.empty(dist.get_world_size() * capacity, DET_ROW, dtype=torch.float32, device=local.device)
    dist.all_gather_into_tensor(out, block)
    return out


def detection_rows_to_coco(rows: torch.Tensor, contiguous_to_dataset_id: Dict[int, int] = None) -> List[Dict[str, Any]]:
    """(n, 8) rows (ONE device->host copy here) -> COCO-json result dicts, boxes XYXY -> XYWH."""
    rows = rows.cpu()
    rows = rows[rows[:, 7] > 0].tolist()
    out = []
    for img_id, x0, y0, x1, y1, s, c, _ in rows:
        cid = int(c)
        out.append({"image_id": int(img_id), "category_id": contiguous_to_dataset_id[cid] if contiguous_to_dataset_id else cid,
                    "bbox": [x0, y0, x1 - x0, y1 - y0], "score": s})
    return out


def detections_to_coco_rows(outputs: List[Dict[str, Any]], image_ids: List[int],
                            contiguous_to_dataset_id: Dict[int, int] = None) -> List[Dict[str, Any]]:
    """COCO-json rows for a whole batch with ONE device->host copy (detections_to_tensor + detection_rows_to_coco)."""
    return detection_rows_to_coco(detections_to_tensor(outputs, image_ids), contiguous_to_dataset_id)
