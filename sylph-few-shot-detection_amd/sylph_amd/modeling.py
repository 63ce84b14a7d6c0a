"""Host-side mirror of the reference's meta-architecture for the inference path.

    model(batched_inputs, class_code=None, run_type=None)

keeps the reference's dispatch, argument meaning and error behaviour
(sylph/modeling/meta_arch/meta_one_stage_detector.py:415-455) while every tensor op runs in
libsylph_hip (one C-ABI call per stage, see sylph_amd/engine.py).  The registries resolve the yaml
names (MODEL.META_ARCHITECTURE "MetaOneStageDetector", MODEL.BACKBONE.NAME
"build_fcos_resnet_fpn_backbone", MODEL.PROPOSAL_GENERATOR.NAME "MetaFCOS",
MODEL.META_LEARN.CODE_GENERATOR.NAME "CodeGenerator" / "ROIEncoder"; sylph/modeling/code_generator/build.py:18-39) to
components the meta-architecture builds, binds to its HIP context and calls where the reference calls the nn.Modules:
another implementation registered under another name plugs in the same way.
"""
import logging
from typing import Any, Dict, List, Optional, Tuple

import torch
from torch import nn

from .engine import Engine, QueryRecord
from .structures import Boxes, Instances
from .views import (DEFAULT_MAX_BATCH, check_views, make_view, plan_view_steps, stitch_params, tta_views, view_merge_route,
                    view_out_size)

logger = logging.getLogger(__name__)


class Registry:
    """name -> object, with the detectron2 Registry surface (register() decorator, get())."""

    def __init__(self, name: str):
        self._name = name
        self._obj_map: Dict[str, Any] = {}

    def register(self, obj: Any = None):
        if obj is None:
            def deco(o):
                self._obj_map[o.__name__] = o
                return o
            return deco
        self._obj_map[obj.__name__] = obj
        return obj

    def get(self, name: str) -> Any:
        if name not in self._obj_map:
            raise KeyError(f"No object named '{name}' found in '{self._name}' registry!")
        return self._obj_map[name]

    def __contains__(self, name: str) -> bool:
        return name in self._obj_map


META_ARCH_REGISTRY = Registry("META_ARCH")
BACKBONE_REGISTRY = Registry("BACKBONE")
PROPOSAL_GENERATOR_REGISTRY = Registry("PROPOSAL_GENERATOR")
CODE_GENERATOR_REGISTRY = Registry("CODE_GENERATOR")


class HipComponent:
    """A registry entry of this package is a real (if thin) component: the meta-architecture builds it from the yaml name, binds it
    to its HIP context and CALLS it where the reference calls the corresponding nn.Module -- so another implementation registered
    under another name (MODEL.BACKBONE.NAME / PROPOSAL_GENERATOR.NAME / CODE_GENERATOR.NAME) is picked up the same way.  The
    tensors stay inside the context (libsylph_hip works on the "current batch"): a component receives host-side arguments and
    returns host-visible results."""

    engine: Optional[Engine] = None

    def bind(self, engine: Engine):
        self.engine = engine
        return self


class FCOSResNetFPNBackbone(HipComponent):
    """convert_batched_inputs_to_image_list + self.backbone(images.tensor) (meta_one_stage_detector.py:174-181,273): normalise,
    pad to size_divisibility, ResNet-FPN + P6/P7.  The pyramid stays in the context as the current batch."""

    size_divisibility = 32

    def __init__(self, cfg, input_shape=None):
        if list(cfg.MODEL.FPN.IN_FEATURES) != ["res3", "res4", "res5"]:
            raise NotImplementedError("FPN.IN_FEATURES must be [res3, res4, res5]")
        if int(cfg.MODEL.FCOS.TOP_LEVELS) != 2:
            raise NotImplementedError("MODEL.FCOS.TOP_LEVELS must be 2 (P6, P7 from p5)")
        if str(cfg.MODEL.FPN.get("NORM", "")) != "":
            raise NotImplementedError("MODEL.FPN.NORM is not supported")
        self.depth = int(cfg.MODEL.RESNETS.DEPTH)

    def __call__(self, images: Optional[List[torch.Tensor]] = None, images_u8: Optional[List[torch.Tensor]] = None,
                 resize_hw=None, rgb_input: bool = False):
        """(3,H,W) float BGR images, or uint8 HWC originals + their ResizeShortestEdge targets (fused input pipeline).
        Returns the per-image (h, w) the network saw (ImageList.image_sizes)."""
        eng = self.engine
        if images_u8 is not None:
            sizes = [(int(s[0]), int(s[1])) for s in resize_hw]
            eng.preprocess_u8(images_u8, sizes, rgb_input=rgb_input)
        else:
            eng.preprocess(images)
            sizes = [(int(im.shape[-2]), int(im.shape[-1])) for im in images]
        eng.backbone()
        return sizes


@BACKBONE_REGISTRY.register()
def build_fcos_resnet_fpn_backbone(cfg, input_shape=None):
    """adet backbone/fpn.py build_fcos_resnet_fpn_backbone as named by the yamls."""
    return FCOSResNetFPNBackbone(cfg, input_shape)


@PROPOSAL_GENERATOR_REGISTRY.register()
class MetaFCOS(HipComponent):
    """MetaFCOS.forward at inference (meta_fcos/fcos.py:140-260): towers + class-conditional classifier on the current pyramid,
    predict_proposals, NMS, detector_postprocess to the requested output sizes."""

    def __init__(self, cfg, input_shape=None):
        pass

    def __call__(self, cls_conv: torch.Tensor, cls_bias: Optional[torch.Tensor], out_sizes, raw: bool = False):
        self.engine.head(cls_conv, cls_bias, raw=raw)
        return self.engine.decode(out_sizes)

    def forward_episodes(self, codes, image_episode, out_sizes):
        """Images of different episodes in one step: image i with codes[image_episode[i]] (Engine.head_episodes)."""
        self.engine.head_episodes(codes, image_episode)
        return self.engine.decode(out_sizes)

    def forward_code_sets(self, codes, out_sizes):
        """Every image against several code sets in one step (Engine.head_code_sets) -> [set][image] detections."""
        self.engine.head_code_sets(codes)
        return self.engine.decode_code_sets(out_sizes)

    def forward_pretrained(self, out_sizes):
        """support_set_per_class_code = None (fcos.py:543-578): the checkpoint's own cls_logits conv, any kernel size the library
        packed (1x1 / 3x3)."""
        self.engine.head_pretrained()
        return self.engine.decode(out_sizes)


def _split_code(code: torch.Tensor, k: int = 1, bias_shape=(1, 1, 1, 1)) -> Dict[str, torch.Tensor]:
    """One packed code row (256 k^2 + 1 floats: cls_conv in torch's (c, ky, kx) order, then the bias) -> the reference's dict."""
    n = 256 * k * k
    return {"cls_conv": code[:n].reshape(1, 256, k, k), "cls_bias": code[n:n + 1].reshape(*bias_shape)}


def _code_dicts(engine, codes: torch.Tensor, k: int = 1, bias_shape=(1, 1, 1, 1), has_scale: bool = False) -> List[Dict[str, torch.Tensor]]:
    """The rows of the codegen* call that `engine` has just made -> one code dict per row; with a SCALE_LAYER each gets the call's
    "cls_weight_norm" (code_generator.py:987-999)."""
    outs = [_split_code(c, k, bias_shape) for c in codes]
    if has_scale:
        for o, w in zip(outs, engine.codegen_weight_norm(len(outs))):
            o["cls_weight_norm"] = w.reshape(1, 1, 1, 1)
    return outs


@CODE_GENERATOR_REGISTRY.register()
class CodeGenerator(HipComponent):
    """CodeGeneratorHead: forward_roi_align on the current support pyramid (code_generator.py:924-1002) and, with cls_norm=True,
    forward_normalize_code over a list of codes (:832-897)."""

    eval_shot = None
    engine_generator = "CodeGenerator"  # which in-library generator (sylph_config.cg_type) this component drives

    def __init__(self, cfg, feature_channels=256, feature_levels=5, strides=None):
        assert feature_channels == 256, "Each level must have the same channel!"
        self.has_scale = len(cfg.MODEL.META_LEARN.CODE_GENERATOR.get("SCALE_LAYER", [])) != 0  # -> "cls_weight_norm" outputs

    def __call__(self, boxes: Optional[torch.Tensor] = None, cls_norm: bool = False, class_codes=None, weight_norm=None):
        if cls_norm:
            return self.engine.normalize_codes(class_codes, weight_norm)
        return self._dicts(self.engine.codegen(boxes)[None])[0]  # cls_conv (1, 256, k, k) with CLS_LAYER kernel size k

    def forward_classes(self, boxes: torch.Tensor, shots: int):
        """Several classes of `shots` support boxes each in the current batch -> one code dict per class (the launches are
        shared, the per-class arithmetic is that of __call__)."""
        return self._dicts(self.engine.codegen_classes(boxes, shots))

    def forward_rois(self, boxes: torch.Tensor, roi_image, seg_len):
        """Classes from a ROI list over the current batch (Engine.codegen_rois): segment j of seg_len[j] (image, box) pairs -> one
        code dict per segment, in forward_classes' shapes.  A segment's arithmetic is that of __call__ on its shots."""
        return self._dicts(self.engine.codegen_rois(boxes, roi_image, seg_len))

    def _dicts(self, codes: torch.Tensor):
        return _code_dicts(self.engine, codes, self.engine.code_ksize, has_scale=self.has_scale)


@CODE_GENERATOR_REGISTRY.register()
class ROIEncoder(HipComponent):
    """ROIEncoder.forward at inference (roi_encoder.py:146-204): one class of EVAL_SHOT support boxes -> its code."""

    engine_generator = "ROIEncoder"

    def __init__(self, cfg, feature_channels=256, feature_levels=5, strides=None):
        assert feature_channels == 256, "Each level must have the same channel!"
        self.eval_shot = int(cfg.MODEL.META_LEARN.EVAL_SHOT)

    def __call__(self, boxes: torch.Tensor):  # no cls_norm / class_codes keywords, like the reference
        return self._dicts(self.engine.codegen(boxes)[None])[0]

    def forward_classes(self, boxes: torch.Tensor, shots: int):
        """Several classes of EVAL_SHOT support boxes each in the current batch -> one code dict per class.  The launches are shared;
        a class's tokens never meet another class's (the reference's encoder sees one class per call at inference: a length-1
        sequence on its attention axis, roi_encoder.py:184-186), so the codes are those of __call__ per class."""
        assert shots == self.eval_shot, f"{shots} support images per class, EVAL_SHOT is {self.eval_shot}"
        return self._dicts(self.engine.codegen_classes(boxes, shots))

    def forward_rois(self, boxes: torch.Tensor, roi_image, seg_len):
        """Classes from a ROI list over the current batch: every segment holds EVAL_SHOT (image, box) pairs -> one code dict per
        segment.  As in forward_classes a segment's tokens never meet another segment's."""
        for j, n in enumerate(seg_len):
            assert int(n) == self.eval_shot, f"segment {j} has {int(n)} ROIs, EVAL_SHOT is {self.eval_shot}"
        return self._dicts(self.engine.codegen_rois(boxes, roi_image, seg_len))

    def _dicts(self, codes: torch.Tensor):
        return _code_dicts(self.engine, codes, bias_shape=(1,))


def build_code_generator(cfg, feature_channels, feature_levels, strides):
    """sylph/modeling/code_generator/build.py:30-39."""
    name = cfg.MODEL.META_LEARN.CODE_GENERATOR.NAME
    return CODE_GENERATOR_REGISTRY.get(name)(cfg, feature_channels, feature_levels, strides)


def check_class_code_args(class_code, class_code_sets):
    """`class_code` and `class_code_sets` of MetaOneStageDetector.forward exclude each other; the sets are a non-empty list of dicts."""
    if class_code_sets is None:
        return None
    if class_code is not None:
        raise ValueError("class_code and class_code_sets were both given: pass the code dict of ONE step as class_code, or the dicts of "
                         "several code sets over the same images as class_code_sets")
    if not isinstance(class_code_sets, (list, tuple)) or len(class_code_sets) == 0:
        raise ValueError("class_code_sets must be a non-empty list of class-code dicts")
    for g, d in enumerate(class_code_sets):
        if not isinstance(d, dict) or "cls_conv" not in d:
            raise ValueError(f"class_code_sets[{g}] is not a class-code dict (no cls_conv)")
    return list(class_code_sets)


def group_episodes(class_code, num_inputs: int):
    """A list / tuple of class-code dicts, one per input -> (the distinct dicts in order of first appearance, episode index per input).
    Entries that are the SAME OBJECT form one episode: equal contents in two dicts are two episodes (nothing is compared)."""
    if len(class_code) != num_inputs:
        raise ValueError(f"class_code has {len(class_code)} entries for {num_inputs} inputs: one class-code dict per input")
    index, dicts, image_episode = {}, [], []
    for i, d in enumerate(class_code):
        if d is None:
            raise ValueError(f"class_code[{i}] is None: pass class_code=None as a whole for the pretrained codes")
        e = index.get(id(d))
        if e is None:
            e = index[id(d)] = len(dicts)
            dicts.append(d)
        image_episode.append(e)
    return dicts, image_episode


RECORD_META_KEYS = ("image_id", "file_name", "height", "width")


def record_input(batched_inputs):
    """The record-input of a model call, or None: `batched_inputs` is then a list of ONE dict {"record": QueryRecord, "inputs": [metadata
    per image]} that stands for the whole batch it was made from (run_type "meta_learn_cache_query")."""
    if not isinstance(batched_inputs, (list, tuple)) or not any(isinstance(x, dict) and "record" in x for x in batched_inputs):
        return None
    if len(batched_inputs) != 1:
        raise ValueError(f"a record input stands for a whole batch: pass a list of exactly one record input, not {len(batched_inputs)} inputs "
                         "(records are not merged, and not mixed with images)")
    x = batched_inputs[0]
    if not isinstance(x["record"], QueryRecord) or len(x.get("inputs", ())) != x["record"].batch[0]:
        raise ValueError("a record input is {'record': QueryRecord, 'inputs': [metadata of each of its images]}")
    return x


@META_ARCH_REGISTRY.register()
class MetaOneStageDetector(nn.Module):
    """Four inference forward types (meta_one_stage_detector.py:415-455):
      run_type None                         -> forward_base_detector for a non-episodic model (plain FCOS with the checkpoint's
                                               cls_logits); NotImplementedError for an episodic model (as the reference)
      "meta_learn_test_support"             -> forward_class_code
      "meta_learn_normalize_code"           -> normalize_class_code
      "meta_learn_test_instance"            -> forward_instances (class_code None: evaluation with the pretrained cls_logits)
                                               class_code a list / tuple of dicts, one per input: images of different episodes
                                               in one step (group_episodes; pred_classes index the image's own dict)
                                               class_code_sets = [d_0, ..., d_{G-1}]: every image against G code sets in one step
                                               -> a list over sets of what class_code=d_g returns (forward_instances_code_sets)
                                               inputs carrying "views" next to "image_u8", or cfg.TEST.AUG.ENABLED: every input is
                                               run on a list of views (crop, size, flip) and the views' detections are merged on the
                                               device (forward_instances_views)
                                               batched_inputs a list of one record-input (below): the same results from the
                                               record's stored tower outputs, without the backbone and the towers
      "meta_learn_cache_query"              -> forward_cache_query: one network pass, no class codes -> [record-input]: a QueryRecord of
                                               the batch with each input's metadata and no image tensors (not in the reference, whose
                                               evaluation pays the whole network per seed and shot setting, meta_fcos_runner.py:451-672)
    Training the network is out of scope: calling the model in training mode raises NotImplementedError.  What is trained here is the
    class-conditional layer alone, on stored tower outputs: `finetune_class_codes` (the TFA baseline; sylph_amd.finetune)."""

    def __init__(self, cfg, dtype: Optional[str] = None, device_index: Optional[int] = None):
        super().__init__()
        self.cfg = cfg
        self.episodic_learning = bool(cfg.MODEL.META_LEARN.EPISODIC_LEARNING)
        self.backbone = BACKBONE_REGISTRY.get(cfg.MODEL.BACKBONE.NAME)(cfg)
        self.proposal_generator = PROPOSAL_GENERATOR_REGISTRY.get(cfg.MODEL.PROPOSAL_GENERATOR.NAME)(cfg)
        self.code_generator = (build_code_generator(cfg, 256, len(cfg.MODEL.FCOS.IN_FEATURES),
                                                    cfg.MODEL.FCOS.FPN_STRIDES) if self.episodic_learning else None)
        if self.episodic_learning:
            assert self.code_generator is not None
        self.in_features = list(cfg.MODEL.FCOS.IN_FEATURES)
        if device_index is None:
            dev = torch.device(cfg.MODEL.DEVICE)
            device_index = dev.index if dev.index is not None else (torch.cuda.current_device() if torch.cuda.is_available() else 0)
        dtype = dtype or str(cfg.MODEL.get("COMPUTE_DTYPE", "bf16"))
        self.engine = Engine(cfg, dtype=dtype, device=device_index)
        for comp in (self.backbone, self.proposal_generator, self.code_generator):
            if hasattr(comp, "bind"):
                comp.bind(self.engine)
        self.register_buffer("pixel_mean", torch.tensor(list(cfg.MODEL.PIXEL_MEAN), dtype=torch.float32,
                                                        device=self.engine.device).view(-1, 1, 1))
        self.register_buffer("pixel_std", torch.tensor(list(cfg.MODEL.PIXEL_STD), dtype=torch.float32,
                                                       device=self.engine.device).view(-1, 1, 1))
        self._weights_loaded = False
        self.train(True)  # nn.Module default; the runner / predictor call .eval()

    # ---- reference surface -------------------------------------------------------------------------
    @property
    def device(self):
        return self.pixel_mean.device

    def load_state_dict(self, state_dict, strict: bool = True):
        """Accepts the reference checkpoint's ["model"] dict (SURVEY.md 8b key layout)."""
        self.engine.load_state_dict(state_dict)
        self._weights_loaded = True
        # the base detector's own classifier (fcos.py:418-427): kept for eval_with_pretrained_code (class_code=None)
        w = state_dict.get("proposal_generator.fcos_head.cls_logits.weight")
        b = state_dict.get("proposal_generator.fcos_head.cls_logits.bias")
        self._pretrained_cls_logits = (torch.as_tensor(w).float(), torch.as_tensor(b).float()) if w is not None and b is not None else None
        return self

    def load_checkpoint(self, path: str):
        """DetectionCheckpointer.load (sylph/predictor.py:87-88): model_final.pth, detectron2 model-zoo .pkl or the MSRA
        R-50.pkl / R-101.pkl backbones the yamls name (sylph_amd.checkpoint maps them onto the reference keys)."""
        from .checkpoint import load_checkpoint_file
        return self.load_state_dict(load_checkpoint_file(path))

    def forward(self, batched_inputs, class_code=None, run_type=None, class_code_sets=None):
        if self.training:
            raise NotImplementedError("training is out of scope of the MI355X inference path; call model.eval()")
        sets = check_class_code_args(class_code, class_code_sets)
        rec = record_input(batched_inputs) if run_type != "meta_learn_normalize_code" else None
        if rec is not None or run_type == "meta_learn_cache_query":
            self._refuse_views_with_records(batched_inputs if rec is None else rec["inputs"])
            if rec is not None and run_type != "meta_learn_test_instance":
                raise ValueError(f"a query record is scored with run_type 'meta_learn_test_instance', not {run_type!r}")
            if run_type == "meta_learn_cache_query":
                return self.forward_cache_query(batched_inputs)
        views = self._input_views(batched_inputs) if run_type == "meta_learn_test_instance" and rec is None else None
        if views is None and run_type == "meta_learn_test_instance" and rec is None and \
                any(isinstance(x, dict) and x.get("max_detections") is not None for x in batched_inputs):
            raise ValueError("\"max_detections\" is the keep count of the merge of an input's views: it needs \"views\" on the inputs or "
                             "TEST.AUG.ENABLED (without views POST_NMS_TOPK_TEST decides)")
        if views is None and run_type == "meta_learn_test_instance" and rec is None and \
                any(isinstance(x, dict) and stitch_params(x.get("stitch")) is not None for x in batched_inputs):
            raise ValueError("\"stitch\" joins what the borders of an input's views cut: it needs \"views\" on the inputs or TEST.AUG.ENABLED")
        if views is not None:
            if sets is not None:
                raise NotImplementedError("class_code_sets together with query views (inputs carrying \"views\", or TEST.AUG.ENABLED) is not "
                                          "supported: run the view list once per code set with class_code")
            return self.forward_instances_views(batched_inputs, class_code, views)
        if sets is not None:
            if run_type != "meta_learn_test_instance":
                raise NotImplementedError(f"class_code_sets belongs to run_type 'meta_learn_test_instance', not {run_type!r}")
            return self.forward_instances_code_sets(batched_inputs, sets)
        if run_type is None:
            # MetaProposalNetwork.forward (meta_one_stage_detector.py:120-141): a non-episodic model is a plain base detector
            if not self.episodic_learning:
                return self.forward_base_detector(batched_inputs)
            raise NotImplementedError(
                "Episodic learning inferrence for image and features is not supported in forward.")
        if run_type == "meta_learn_test_support":
            return self.forward_class_code(batched_inputs)
        if run_type == "meta_learn_normalize_code":
            return self.normalize_class_code(class_code)
        if run_type == "meta_learn_test_instance":
            return self.forward_instances(batched_inputs, class_code)
        raise NotImplementedError(f"not support this forward type: {run_type}, class_code: {class_code}")

    # ---- support path --------------------------------------------------------------------------------
    def forward_class_code(self, batched_inputs: List[Dict[str, Any]]) -> Dict[str, torch.Tensor]:
        """meta_one_stage_detector.py:229-254: ONE class, its S support records."""
        assert not self.training, "Not for training"
        assert len(batched_inputs) == 1, f"batched_inputs has length: {len(batched_inputs)}"
        records = [rec for x in batched_inputs for rec in x["support_set"]]
        boxes = []
        for rec in records:
            gt = rec["instances"].gt_boxes.tensor
            if len(gt) == 0:  # select_a_mask (code_generator/utils.py:35-38)
                logger.info("Run into empty box, use zero masks")
                raise ValueError
            if len(gt) > 1:
                # the reference draws np.random.choice here (global RNG, utils.py:41); deterministic
                # only when one box is given -- we require the caller to have selected it
                import numpy as np
                gt = gt[np.random.choice(range(len(gt)), 1)]
            boxes.append(gt.reshape(1, 4))
        num_shots = getattr(self.code_generator, "eval_shot", None)
        if num_shots:
            # roi_encoder.py:156-166: num_shots = EVAL_SHOT in eval, batch = total / num_shots (one class here)
            assert len(records) % num_shots == 0, f"{len(records)} % {num_shots}"
            assert len(records) // num_shots == 1, "one class per call at inference"
        self.backbone(images=[rec["image"] for rec in records])
        return self.code_generator(torch.cat(boxes, dim=0))

    def forward_class_codes(self, items: List[List[Dict[str, Any]]]) -> List[Dict[str, torch.Tensor]]:
        """Support-path throughput: the reference (and forward_class_code above) runs ONE class per call; here several classes
        share the backbone / code-generator launches of one batch (B = classes x shots).  `items`: loader items, each a list of
        length 1 as in forward_class_code.  Falls back to one call per class when the shot counts differ (or are not the
        ROIEncoder's EVAL_SHOT), a record carries more than one box, or the classes would be padded to different sizes when run
        alone (the padded size decides the activations along the right / bottom border, hence the code)."""
        assert not self.training, "Not for training"
        recs = [[rec for x in it for rec in x["support_set"]] for it in items]
        shots = len(recs[0]) if recs else 0
        from .evaluation import class_padded_hw
        d = getattr(self.backbone, "size_divisibility", 32)
        batchable = (len(items) > 1 and hasattr(self.code_generator, "forward_classes") and shots > 0
                     and getattr(self.code_generator, "eval_shot", None) in (None, shots)
                     and len({class_padded_hw(r, d) for r in recs if r}) == 1  # every class padded as in its own one-class call
                     and all(len(it) == 1 and len(r) == shots for it, r in zip(items, recs))
                     and all(len(rec["instances"].gt_boxes.tensor) == 1 for r in recs for rec in r))
        if not batchable:
            return [self.forward_class_code(it) for it in items]
        self.backbone(images=[rec["image"] for r in recs for rec in r])
        boxes = torch.cat([rec["instances"].gt_boxes.tensor.reshape(1, 4) for r in recs for rec in r], dim=0)
        return self.code_generator.forward_classes(boxes, shots)

    def forward_class_codes_rois(self, records: List[Dict[str, Any]], segments: List[Dict[str, torch.Tensor]]) -> List[Dict[str, torch.Tensor]]:
        """Class codes from annotated images at ONE backbone pass per image: `records` are the B images of the batch (dicts with
        "image"), `segments` a list of {"image_index": LongTensor(n), "boxes": Tensor(n, 4)}: the n support instances of one class
        (or one chunk of a class), instance i being box boxes[i] on records[image_index[i]], in network-input coordinates like
        gt_boxes.  Returns one code dict per segment in forward_class_code's format; a segment's code is forward_class_code's on a
        support set that repeats each image once per instance.  Every given instance counts: nothing is drawn at random."""
        assert not self.training, "Not for training"
        assert self.episodic_learning and hasattr(self.code_generator, "forward_rois")
        boxes, roi_image, seg_len = [], [], []
        for j, seg in enumerate(segments):
            idx = torch.as_tensor(seg["image_index"]).reshape(-1).tolist()
            bx = torch.as_tensor(seg["boxes"]).reshape(-1, 4)
            if len(idx) == 0:
                raise ValueError(f"segment {j} is empty: a class needs at least one support instance")
            if len(idx) != bx.shape[0]:
                raise ValueError(f"segment {j} has {len(idx)} image indices for {bx.shape[0]} boxes")
            for i in idx:
                if i < 0 or i >= len(records):
                    raise ValueError(f"segment {j}: image_index {i} is outside the {len(records)} records")
            boxes.append(bx.float().cpu())
            roi_image.extend(int(i) for i in idx)
            seg_len.append(len(idx))
        if not segments:
            raise ValueError("no segments")
        self.backbone(images=[rec["image"] for rec in records])
        return self.code_generator.forward_rois(torch.cat(boxes, dim=0), roi_image, seg_len)

    def forward_shot_rows(self, records: List[Dict[str, Any]]):
        """Shot-bank rows of annotated images at ONE backbone pass per image: every annotated instance of `records` (dicts with "image"
        and "instances" carrying gt_boxes / gt_classes), in record order, then box order -> (rows (R, shot_row_floats) on the device,
        image_index [R], ann_index [R], class_ids [R]); (None, [], [], []) when no record carries a box.  Row r is everything
        forward_class_codes_rois computes from instance r alone (Engine.codegen_shots); Engine.combine_shots makes the code of any
        list of such rows.  Nothing is drawn at random."""
        assert not self.training, "Not for training"
        assert self.episodic_learning and self.code_generator is not None
        boxes, image_index, ann_index, class_ids = [], [], [], []
        for b, rec in enumerate(records):
            inst = rec.get("instances")
            if inst is None or len(inst.gt_boxes.tensor) == 0:
                continue
            gt = inst.gt_boxes.tensor.detach().float().cpu().reshape(-1, 4)
            cls = torch.as_tensor(inst.gt_classes).reshape(-1).tolist()
            assert len(cls) == gt.shape[0], f"record {b}: {len(cls)} classes for {gt.shape[0]} boxes"
            boxes.append(gt)
            image_index += [b] * len(cls)
            ann_index += list(range(len(cls)))
            class_ids += [int(c) for c in cls]
        if not boxes:
            return None, [], [], []
        self.backbone(images=[rec["image"] for rec in records])
        return self.engine.codegen_shots(torch.cat(boxes, dim=0), image_index), image_index, ann_index, class_ids

    def forward_roi_rows(self, records: List[Dict[str, Any]]):
        """ROI-bank rows of annotated images at ONE backbone pass per image: every annotated instance of `records`, in record order, then
        box order -> (rows (R, 49, 256) bf16 on the device, class_ids [R]); (None, []) when no record carries a box (Engine.roi_rows)."""
        assert not self.training, "Not for training"
        boxes, image_index, class_ids = [], [], []
        for b, rec in enumerate(records):
            inst = rec.get("instances")
            if inst is None or len(inst.gt_boxes.tensor) == 0:
                continue
            gt = inst.gt_boxes.tensor.detach().float().cpu().reshape(-1, 4)
            cls = torch.as_tensor(inst.gt_classes).reshape(-1).tolist()
            assert len(cls) == gt.shape[0], f"record {b}: {len(cls)} classes for {gt.shape[0]} boxes"
            boxes.append(gt)
            image_index += [b] * len(cls)
            class_ids += [int(c) for c in cls]
        if not boxes:
            return None, []
        self.backbone(images=[rec["image"] for rec in records])
        return self.engine.roi_rows(torch.cat(boxes, dim=0), image_index), class_ids

    def train_code_generator(self, bank, records, annotations, **kw):
        """Meta-train the code generator on the frozen detector (sylph_amd.metatrain.train_code_generator; kw: iters, classes_per_step,
        shots, records_per_step, lr, clip_norm, momentum, weight_decay, lr_steps, lr_gamma, trainable, seed).  Returns (state_dict,
        losses); set_code_generator installs the state dict."""
        from .metatrain import train_code_generator
        return train_code_generator(self, bank, records, annotations, **kw)

    def set_code_generator(self, state):
        """Install a trained generator (train_code_generator's state dict, a flat vector, or None for the checkpoint's) into the serving
        path (Engine.set_code_generator): shot banks built under another generator are refused from then on."""
        self.engine.set_code_generator(state)

    def normalize_class_code(self, codes: List[Dict]):
        """code_generator.py:877-897 via meta_one_stage_detector.py:256-259 (mutates the list)."""
        assert self.episodic_learning
        assert not self.training
        if isinstance(self.code_generator, ROIEncoder):
            # the reference fails the same way: ROIEncoder.forward() takes no cls_norm/class_codes
            # (meta_one_stage_detector.py:259 -> roi_encoder.py:146)
            raise TypeError("ROIEncoder.forward() got an unexpected keyword argument 'cls_norm'")
        assert codes is not None
        if len(codes) == 0:
            return codes
        rows, wns = [], []
        for code in codes:
            assert "class_code" in code, "class_code is not in code"
            assert "cls_conv" in code["class_code"], "class_conv is not in class_code"
            cc = code["class_code"]
            assert cc["cls_conv"].ndim == 4
            k = self.engine.code_ksize
            if tuple(cc["cls_conv"].shape[1:]) != (256, k, k):
                raise ValueError(f"class code of shape {tuple(cc['cls_conv'].shape)}: this model normalises {k}x{k} codes "
                                 f"(1, 256, {k}, {k}) (CODE_GENERATOR.CLS_LAYER kernel size {k})")
            assert cc["cls_bias"].numel() == 1, "predicted bias should only have batch size 1"
            rows.append(torch.cat([cc["cls_conv"].reshape(-1).float(), cc["cls_bias"].reshape(-1).float()]))
            if "cls_weight_norm" in cc:  # x cls_weight_norm after the L2 normalisation (code_generator.py:838-840)
                wns.append(cc["cls_weight_norm"].reshape(-1).float())
        assert len(wns) in (0, len(rows)), "cls_weight_norm must be present for all classes or none"
        packed = torch.stack(rows).to(self.device).contiguous()
        out = self.code_generator(cls_norm=True, class_codes=packed, weight_norm=torch.cat(wns) if wns else None)
        for i, code in enumerate(codes):
            code["class_code"].update(_split_code(out[i], self.engine.code_ksize, bias_shape=(1,)))
        return codes

    # ---- query path ----------------------------------------------------------------------------------
    def forward_base_detector(self, batched_inputs: List[Dict[str, Any]]):
        """meta_one_stage_detector.py:298-323 (inference branch) + the {"proposals"} -> {"instances"} renaming of
        MetaOneStageDetector.forward (:436-441): FCOS with the checkpoint's own cls_logits."""
        assert not self.episodic_learning
        return self._detect(batched_inputs, None)

    def forward_instances(self, batched_inputs: List[Dict[str, Any]], class_codes: Dict[str, torch.Tensor]):
        """meta_one_stage_detector.py:261-296 -> [{"instances": Instances}] at input["height"/"width"] scale."""
        assert self.episodic_learning
        return self._detect(batched_inputs, class_codes)

    def forward_instances_code_sets(self, batched_inputs: List[Dict[str, Any]], class_code_sets: List[Dict[str, torch.Tensor]]):
        """The query batch against G code sets at ONE backbone / tower pass (sylph_fcos_head_codesets): the G query passes of the
        TEST.REPEAT_TEST protocol (meta_fcos_runner.py:451-672) or G tenants of one frame -> [forward_instances(batch, d_g) for d_g]."""
        assert self.episodic_learning
        assert not self.training, "Not for training"
        codes = [(d["cls_conv"], d.get("cls_bias")) for d in class_code_sets]
        for w, _ in codes:
            assert w.dim() == 4, f"Weight has dimension: {w.dim()}"
            assert w.size(1) == 256
        out_sizes = self._run_backbone(batched_inputs)
        return [self._to_results(d, out_sizes) for d in self.proposal_generator.forward_code_sets(codes, out_sizes)]

    def _detect(self, batched_inputs: List[Dict[str, Any]], class_codes):
        assert not self.training, "Not for training"
        if isinstance(class_codes, (list, tuple)):
            # one class-code dict per input: the images of several episodes share one step (sylph_fcos_head_episodes); pred_classes
            # index the image's own dict
            rec = record_input(batched_inputs)
            dicts, image_episode = group_episodes(class_codes, len(batched_inputs) if rec is None else len(rec["inputs"]))
            codes = [(d["cls_conv"], d.get("cls_bias")) for d in dicts]
            for w, _ in codes:
                assert w.dim() == 4, f"Weight has dimension: {w.dim()}"
                assert w.size(1) == 256
            out_sizes = self._run_backbone(batched_inputs)
            return self._to_results(self.proposal_generator.forward_episodes(codes, image_episode, out_sizes), out_sizes)
        pretrained = class_codes is None
        if class_codes is None:
            class_codes = self._pretrained_class_codes()
        w, b = class_codes["cls_conv"], class_codes.get("cls_bias")
        assert w.dim() == 4, f"Weight has dimension: {w.dim()}"
        assert w.size(1) == 256
        conv3 = pretrained and tuple(w.shape[2:]) == (3, 3)  # a 3x3 cls_logits is a real conv, not a class-conditional 1x1
        out_sizes = self._run_backbone(batched_inputs)
        # the checkpoint's own cls_logits are a plain conv: no CondConvBlock Scale on a ROIEncoder model
        if conv3:
            dets = self.proposal_generator.forward_pretrained(out_sizes)
        else:
            dets = self.proposal_generator(w, b, out_sizes, raw=True) if pretrained else self.proposal_generator(w, b, out_sizes)
        return self._to_results(dets, out_sizes)

    def _pretrained_class_codes(self) -> Dict[str, torch.Tensor]:
        """class_code None: the checkpoint's own classifier as a code dict"""
        # MetaFCOSHead.forward with support_set_per_class_code=None -> forward_base_train (fcos.py:543-578):
        # logits = self.cls_logits(cls_tower), the pretrained base-class classifier.  A 1x1 cls_logits conv (the
        # CLS_LOGITS_KERNEL_SIZE of the Meta-FCOS recipes) is exactly the class-conditional conv with fixed codes.
        pre = getattr(self, "_pretrained_cls_logits", None)
        if pre is None:
            raise ValueError("class_code is None and the checkpoint has no proposal_generator.fcos_head.cls_logits weights")
        if pre[0].dim() != 4 or tuple(pre[0].shape[2:]) not in ((1, 1), (3, 3)):
            raise NotImplementedError(f"pretrained cls_logits with kernel {tuple(pre[0].shape[2:])}: only 1x1 and 3x3 "
                                      "(MODEL.FCOS.CLS_LOGITS_KERNEL_SIZE) are supported")
        if self.episodic_learning and not bool(self.cfg.MODEL.META_LEARN.CODE_GENERATOR.USE_BIAS):
            raise NotImplementedError("pretrained cls_logits needs the bias path of the class-conditional conv (USE_BIAS)")
        return {"cls_conv": pre[0].to(self.device), "cls_bias": pre[1].to(self.device)}

    # ---- query views: test-time augmentation and tiled images ----------------------------------------------
    view_max_batch = DEFAULT_MAX_BATCH  # views per step (plan_view_steps)

    def _input_views(self, batched_inputs: List[Dict[str, Any]]):
        """The view list of every input, or None when the batch has none: no input carries "views" and TEST.AUG.ENABLED is off.
        An input's own "views" win; with TEST.AUG.ENABLED the others get detectron2's DatasetMapperTTA list (tta_views); without it an
        input that has no views next to inputs that have some is one full-frame view at its "resize_hw"."""
        cfg = getattr(self, "cfg", None)
        aug = cfg.get("TEST", {}).get("AUG", {}) if hasattr(cfg, "get") else {}
        enabled = bool(aug.get("ENABLED", False))
        if not enabled and not any("views" in x for x in batched_inputs):
            return None
        out = []
        for i, x in enumerate(batched_inputs):
            if "image_u8" not in x:
                why = "TEST.AUG.ENABLED" if enabled and "views" not in x else "an input with \"views\""
                raise ValueError(f"input {i}: {why} needs the original uint8 image as \"image_u8\" (the views are cut from it on the device); "
                                 "a float \"image\" has already been resized")
            h, w = int(x["image_u8"].shape[0]), int(x["image_u8"].shape[1])
            if "views" in x:
                out.append(check_views(x["views"], h, w, f"input {i}: views"))
            elif enabled:
                out.append(tta_views(h, w, [int(s) for s in aug.MIN_SIZES], int(aug.MAX_SIZE), bool(aug.FLIP)))
            else:
                out.append([make_view((0, 0, w, h), x["resize_hw"])])
        return out

    def forward_instances_views(self, batched_inputs: List[Dict[str, Any]], class_codes, per_input_views):
        """Every input on its views, merged per input: the views of the whole batch are planned into steps by resize target
        (plan_view_steps); a step is preprocess_views (cut from the sources, which are uploaded once) -> backbone -> head -> decode at
        the crop size into its slice of one row buffer; then ONE merge call (class-wise NMS over the views of a source, in source
        pixels; views.merge_route picks the one-block merge or, for a source of more than 4 096 rows or a "max_detections" = K on the
        inputs, the workspace merge with K as rule 5's count and 2 K output rows; with "stitch" on the inputs, Engine.stitch_views, which
        also joins what tile borders cut and adds the field `stitched`) and one read-back.  class_codes: a dict (every
        view), a per-input list (all views of an input take its episode) or None (the pretrained classifier).  -> [{"instances": Instances}] at the source's size, or at "height" / "width" when they differ
        (rescaled and clipped as detector_postprocess does) with pred_boxes, scores, pred_classes and the provenance view_index (into the
        input's own view list) / view_row."""
        assert not self.training, "Not for training"
        eng = self.engine
        topk = self._max_detections(batched_inputs)
        stitch = self._stitch(batched_inputs)
        run_head = self._view_head(class_codes, len(batched_inputs))
        table = [dict(v, source=i, view=k) for i, vs in enumerate(per_input_views) for k, v in enumerate(vs)]
        steps = plan_view_steps(table, int(self.view_max_batch), int(getattr(self.backbone, "size_divisibility", 32)))
        table = [table[i] for st in steps for i in st]  # view index = row of the buffer: step after step
        sources = [x["image_u8"].to(self.device, non_blocking=True).contiguous() for x in batched_inputs]
        rgb = str(batched_inputs[0].get("input_format", "BGR")) == "RGB"
        rows = eng.new_view_rows(len(table))
        row0 = 0
        for st in steps:
            vs = table[row0:row0 + len(st)]
            eng.preprocess_views(sources, vs, rgb_input=rgb)
            eng.backbone()
            run_head([v["source"] for v in vs])
            eng.decode_rows(rows, row0, [view_out_size(v) for v in vs])
            row0 += len(st)
        results = []
        own_index = torch.tensor([v["view"] for v in table], device=self.device)  # row of the buffer -> index in the input's own view list
        per_source = [len(vs) for vs in per_input_views]
        route = view_merge_route(per_source, rows["max_in"], topk, stitch)
        if route == "block":
            merged = eng.merge_views(table, rows, n_src=len(batched_inputs))
        elif route == "stitch":
            merged = eng.stitch_views(table, rows, [(int(s.shape[0]), int(s.shape[1])) for s in sources], stitch[0], stitch[1],
                                      max_out=None if topk is None else 2 * topk, n_src=len(batched_inputs), topk=topk)
        else:  # a K of the inputs' own replaces the config's for the merged result only: every view was decoded under the config
            merged = eng.merge_views_large(table, rows, max_out=None if topk is None else 2 * topk, n_src=len(batched_inputs), topk=topk)
        for x, src, d in zip(batched_inputs, sources, merged):
            h, w = int(src.shape[0]), int(src.shape[1])
            H, W = int(x.get("height", h)), int(x.get("width", w))
            boxes, scores, classes = d["pred_boxes"], d["scores"], d["pred_classes"]
            view_index, view_row = own_index[d["view_index"]], d["view_row"]
            stitched = d.get("stitched")
            if (H, W) != (h, w):  # detector_postprocess: scale, clip, drop what became empty
                boxes = boxes * boxes.new_tensor([W / w, H / h, W / w, H / h])
                boxes = torch.minimum(boxes.clamp(min=0), boxes.new_tensor([W, H, W, H]))
                keep = ((boxes[:, 2] - boxes[:, 0]) > 0) & ((boxes[:, 3] - boxes[:, 1]) > 0)
                boxes, scores, classes, view_index, view_row = boxes[keep], scores[keep], classes[keep], view_index[keep], view_row[keep]
                stitched = stitched[keep] if stitched is not None else None
            r = Instances((H, W))
            r.pred_boxes = Boxes(boxes)
            r.scores = scores
            r.pred_classes = classes
            r.view_index = view_index  # which of the input's views each detection came from, and its row in that view's decode
            r.view_row = view_row
            if stitched is not None:
                r.stitched = stitched  # the rows this detection stands for, itself included (1: nothing was joined to it)
            results.append({"instances": r})
        return results

    @staticmethod
    def _stitch(batched_inputs: List[Dict[str, Any]]) -> Optional[Tuple[float, float]]:
        """The "stitch" of a batch with views -> (stitch_thr, border_px), None when no input asks for it.  One merge call has one pair."""
        ps = {stitch_params(x.get("stitch")) for x in batched_inputs}
        if len(ps) > 1:
            raise ValueError(f"the inputs of one batch disagree on \"stitch\": {sorted(ps, key=lambda p: (p is not None, p))}")
        return ps.pop()

    @staticmethod
    def _max_detections(batched_inputs: List[Dict[str, Any]]) -> Optional[int]:
        """The "max_detections" of a batch with views: rule 5's K of the merge, None when no input carries one.  One merge call has one K."""
        ks = {int(x["max_detections"]) if x.get("max_detections") is not None else None for x in batched_inputs}
        if len(ks) > 1:
            raise ValueError(f"the inputs of one batch disagree on \"max_detections\": {sorted(ks, key=lambda k: (k is not None, k))}")
        k = ks.pop()
        if k is not None and k <= 0:
            raise ValueError(f"\"max_detections\" must be a positive count, got {k}")
        return k

    def _view_head(self, class_codes, num_inputs: int):
        """-> run(view_sources): the head on the current batch of views, view b belonging to input view_sources[b]"""
        eng = self.engine
        if isinstance(class_codes, (list, tuple)):
            dicts, input_episode = group_episodes(class_codes, num_inputs)
            codes = [(d["cls_conv"], d.get("cls_bias")) for d in dicts]
            for w, _ in codes:
                assert w.dim() == 4, f"Weight has dimension: {w.dim()}"
                assert w.size(1) == 256
            return lambda view_sources: eng.head_episodes(codes, [input_episode[s] for s in view_sources])
        pretrained = class_codes is None
        if pretrained:
            class_codes = self._pretrained_class_codes()
        w, b = class_codes["cls_conv"], class_codes.get("cls_bias")
        assert w.dim() == 4, f"Weight has dimension: {w.dim()}"
        assert w.size(1) == 256
        if pretrained and tuple(w.shape[2:]) == (3, 3):
            return lambda view_sources: eng.head_pretrained()
        return lambda view_sources: eng.head(w, b, raw=pretrained)

    def _refuse_views_with_records(self, inputs):
        cfg = getattr(self, "cfg", None)
        aug = cfg.get("TEST", {}).get("AUG", {}) if hasattr(cfg, "get") else {}
        if bool(aug.get("ENABLED", False)):
            raise NotImplementedError("query records with TEST.AUG.ENABLED are not supported: a record holds one batch as the network saw it, "
                                      "not the views of its inputs")
        if any("views" in x for x in inputs):
            raise NotImplementedError("query records of inputs that carry \"views\" are not supported: a record holds one batch as the network "
                                      "saw it, not the views of its inputs")

    def forward_cache_query(self, batched_inputs: List[Dict[str, Any]]):
        """One network pass over the query batch with no class codes -> [{"record": QueryRecord, "inputs": [...]}]: what the towers left
        (Engine.store_record) and, per input, image_id / file_name / height / width and the size the network saw ("net_height",
        "net_width") -- no image tensors.  Passed back as batched_inputs of a "meta_learn_test_instance" call, with class_code or
        class_code_sets, it gives what that call gives on `batched_inputs`.  The caller owns the record (close() releases its bytes)."""
        assert not self.training, "Not for training"
        out_sizes, net_sizes = self._run_backbone(batched_inputs, with_net_sizes=True)
        self.engine.towers()
        rec = self.engine.store_record()
        metas = []
        for x, (oh, ow), (nh, nw) in zip(batched_inputs, out_sizes, net_sizes):
            m = {k: x[k] for k in RECORD_META_KEYS if k in x}
            m.update(height=oh, width=ow, net_height=nh, net_width=nw)
            metas.append(m)
        return [{"record": rec, "inputs": metas}]

    # ---- fine-tuning the class codes on annotated images (the TFA baseline; sylph_amd.finetune) --------------------------------------
    @staticmethod
    def _record_annotations(rec_input) -> Dict[str, torch.Tensor]:
        """boxes / classes / image_index of one record-input whose per-image metadata carries "instances".  gt_boxes live in the frame
        instances.image_size names; they are scaled to the size the network saw (net_height, net_width)."""
        boxes, classes, index = [], [], []
        for i, m in enumerate(rec_input["inputs"]):
            inst = m.get("instances")
            if inst is None:
                raise ValueError(f"finetune_class_codes: input {i} of a record carries no \"instances\"")
            bx = inst.gt_boxes.tensor.detach().float().cpu().reshape(-1, 4)
            ih, iw = inst.image_size
            nh, nw = int(m.get("net_height", ih)), int(m.get("net_width", iw))
            if (nh, nw) != (int(ih), int(iw)):
                bx = bx * torch.tensor([nw / iw, nh / ih, nw / iw, nh / ih])
            boxes.append(bx)
            classes.append(inst.gt_classes.detach().cpu().reshape(-1).long())
            index.append(torch.full((bx.shape[0],), i, dtype=torch.long))
        return {"boxes": torch.cat(boxes), "classes": torch.cat(classes), "image_index": torch.cat(index)}

    def finetune_class_codes(self, batched_inputs, class_code=None, *, batch_size: Optional[int] = None, **kw):
        """Refine `class_code` on annotated images (sylph_amd.finetune.finetune_class_codes; kw: iters, lr, momentum, weight_decay,
        records_per_step, trainable, lr_steps, lr_gamma, seed).  `batched_inputs`: dicts with "image" (or "image_u8" + "resize_hw") and
        "instances" -- one network pass per `batch_size` of them makes the records, which are released at the end -- or record-inputs
        of "meta_learn_cache_query" whose per-image metadata was given "instances".  `class_code`: the dict of "meta_learn_test_support" +
        "meta_learn_normalize_code", or None for the checkpoint's own cls_logits rows (a base detector).  Returns (class codes for
        "meta_learn_test_instance", the loss of every step as one device tensor)."""
        from .finetune import finetune_class_codes
        assert not self.training, "call model.eval(): only the class codes are trained, by their own optimiser"
        if class_code is None:
            class_code = self._pretrained_class_codes()
        inputs = list(batched_inputs)
        is_rec = [isinstance(x, dict) and "record" in x for x in inputs]
        if any(is_rec) and not all(is_rec):
            raise ValueError("finetune_class_codes: records are not mixed with images")
        own = []
        try:
            if not any(is_rec):
                bs = int(batch_size) if batch_size else max(len(inputs), 1)
                rec_inputs = []
                for i in range(0, len(inputs), bs):
                    chunk = inputs[i:i + bs]
                    r = self.forward_cache_query(chunk)[0]
                    own.append(r["record"])
                    for m, x in zip(r["inputs"], chunk):
                        m["instances"] = x["instances"]
                    rec_inputs.append(r)
            else:
                rec_inputs = inputs
            return finetune_class_codes(self, [r["record"] for r in rec_inputs], [self._record_annotations(r) for r in rec_inputs],
                                        class_code, **kw)
        finally:
            for r in own:
                r.close()

    # ---- fine-tuning the box branch on annotated images (the tfa-finetune yamls; sylph_amd.finetune.finetune_box_branch) ---------------
    def box_samples_of(self, batched_inputs, *, batch_size: Optional[int] = 16):
        """The box-sample bank of annotated images (dicts with "image" or "image_u8" + "resize_hw", and "instances"): one network pass
        per `batch_size` of them, the samples of every pass collected while its bbox tower output is fresh."""
        from .engine import BoxSamples
        assert not self.training, "call model.eval(): only the box branch is trained, by its own optimiser"
        inputs = list(batched_inputs)
        if any(isinstance(x, dict) and "record" in x for x in inputs):
            raise ValueError("finetune_box_branch: a query record holds no bbox tower; pass the annotated images themselves")
        bs = int(batch_size) if batch_size else max(len(inputs), 1)
        banks = []
        for i in range(0, len(inputs), bs):
            chunk = inputs[i:i + bs]
            out_sizes, net_sizes = self._run_backbone(chunk, with_net_sizes=True)
            self.engine.towers()
            metas = [dict(instances=x["instances"], net_height=nh, net_width=nw) for x, (nh, nw) in zip(chunk, net_sizes)]
            ann = self._record_annotations({"inputs": metas})
            banks.append(self.engine.box_samples(ann["boxes"], ann["classes"], ann["image_index"]))
        return BoxSamples.cat(banks)

    def finetune_box_branch(self, batched_inputs, *, batch_size: Optional[int] = 16, **kw):
        """Train the box branch (bbox_pred, ctrness, iou_overlap, the level scales) on annotated images: the samples are collected by
        `box_samples_of`, then sylph_amd.finetune.finetune_box_branch runs from the branch the engine runs now (kw: iters, lr, momentum,
        weight_decay, lr_steps, lr_gamma, samples_per_step, seed).  Returns (branch, losses); `set_box_branch` installs the branch."""
        from .finetune import finetune_box_branch
        samples = self.box_samples_of(batched_inputs, batch_size=batch_size)
        return finetune_box_branch(self.engine, samples, self.engine.box_branch(), **kw)

    def set_box_branch(self, branch):
        """Install a box branch for every later pass (None: the checkpoint's).  Query records made under another branch are refused."""
        self.engine.set_box_branch(branch)

    def _run_backbone(self, batched_inputs: List[Dict[str, Any]], with_net_sizes: bool = False):
        """preprocess + backbone of the query batch -> the (height, width) each image's detections are scaled to.  A record-input: no
        network at all, its record becomes the current batch and the sizes are the stored ones."""
        rec = record_input(batched_inputs)
        if rec is not None:
            self.engine.load_record(rec["record"])
            return [(int(m["height"]), int(m["width"])) for m in rec["inputs"]]
        if all("image_u8" in x for x in batched_inputs):
            # fused input pipeline: the original uint8 HWC image + its ResizeShortestEdge target; resize,
            # BGR conversion, normalisation and padding run in one HIP kernel (sylph_preprocess_u8)
            sizes = self.backbone(images_u8=[x["image_u8"] for x in batched_inputs], resize_hw=[x["resize_hw"] for x in batched_inputs],
                                  rgb_input=str(batched_inputs[0].get("input_format", "BGR")) == "RGB")
        else:
            sizes = self.backbone(images=[x["image"] for x in batched_inputs])
        out = [(int(x.get("height", s[0])), int(x.get("width", s[1]))) for x, s in zip(batched_inputs, sizes)]
        return (out, [(int(s[0]), int(s[1])) for s in sizes]) if with_net_sizes else out

    @staticmethod
    def _to_results(dets, out_sizes):
        results = []
        for d, osz in zip(dets, out_sizes):
            r = Instances(osz)
            r.pred_boxes = Boxes(d["pred_boxes"])
            r.scores = d["scores"]
            r.pred_classes = d["pred_classes"]
            r.locations = d["locations"]
            r.fpn_levels = d["fpn_levels"]
            results.append({"instances": r})
        return results


def build_model(cfg, dtype: Optional[str] = None) -> nn.Module:
    """d2go runner.build_model equivalent for this path: META_ARCH_REGISTRY lookup by yaml name."""
    return META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE)(cfg, dtype=dtype)
