"""Thin Python handle over one libsylph_hip context (one per process / GPU).

Tensors are torch CUDA(ROCm) tensors used purely as device-memory owners: every stage below is one
call through the C ABI (include/sylph_hip.h) into hand-written HIP kernels.
"""
import ctypes
import os
from ctypes import c_int, c_int64, c_void_p
from typing import Any, Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import SylphConfig, check


def _ptr(t: Optional[torch.Tensor]):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


def _env_int(name: str, default: int) -> int:
    """an integer SYLPH_* environment override as the library reads it (knob_env): `default` when unset or not a number"""
    try:
        return int(os.environ.get(name, default))
    except ValueError:
        return default


def _iarr(v: Sequence[int]):
    return (c_int * len(v))(*[int(x) for x in v])


def _check_resnet_keys(sc, r, basic):
    """The MODEL.RESNETS keys of a detectron2 ResNet bottom-up that change the graph and are not implemented (MobileNetV2 reads none)."""
    if any(bool(v) for v in r.get("DEFORM_ON_PER_STAGE", [False] * 4)):
        raise NotImplementedError("MODEL.RESNETS.DEFORM_ON_PER_STAGE: deformable bottleneck convs are not supported")
    if int(r.get("RES5_DILATION", 1)) != 1:
        raise NotImplementedError("MODEL.RESNETS.RES5_DILATION != 1 is not supported")
    res2_out = int(r.get("RES2_OUT_CHANNELS", 256))
    if basic and res2_out != 64:
        raise NotImplementedError(f"MODEL.RESNETS.RES2_OUT_CHANNELS {res2_out}: DEPTH {sc.resnet_depth} (BasicBlock) needs RES2_OUT_CHANNELS 64")
    if not basic and res2_out == 64:
        raise NotImplementedError(f"MODEL.RESNETS.RES2_OUT_CHANNELS 64 belongs to DEPTH 18 / 34 (BasicBlock); DEPTH {sc.resnet_depth} needs 256")
    if res2_out != (64 if basic else 256) or int(r.get("STEM_OUT_CHANNELS", 64)) != 64:
        raise NotImplementedError("MODEL.RESNETS.RES2_OUT_CHANNELS / STEM_OUT_CHANNELS: only 256 (64 for DEPTH 18 / 34) / 64 are supported")
    if str(r.get("NORM", "FrozenBN")) != "FrozenBN":
        raise NotImplementedError(f"MODEL.RESNETS.NORM {r.NORM!r}: only FrozenBN (inference) is supported")


def config_from_cfg(cfg) -> SylphConfig:
    """Map the yacs node (sylph_amd.config / the reference's keys) onto the C config struct."""
    L = _lib.lib()
    sc = SylphConfig()
    L.sylph_config_default(ctypes.byref(sc))
    if cfg is None:
        return sc
    m = cfg.MODEL
    f = m.FCOS
    # adet's build_fcos_resnet_fpn_backbone picks the bottom-up path in this order: BACKBONE.ANTI_ALIAS (low-pass-filtered ResNet),
    # RESNETS.DEFORM_INTERVAL > 1 (interval-deformable ResNet), MODEL.MOBILENET (MobileNetV2), else detectron2's ResNet.  The first two
    # are not implemented and win over MOBILENET there, so they refuse here whatever MOBILENET says.
    bb = m.get("BACKBONE", None)
    if bb is not None and bool(bb.get("ANTI_ALIAS", False)):
        raise NotImplementedError("MODEL.BACKBONE.ANTI_ALIAS: the anti-aliased (low-pass-filtered) ResNet is not supported")
    if int(m.RESNETS.get("DEFORM_INTERVAL", 1)) > 1:
        raise NotImplementedError("MODEL.RESNETS.DEFORM_INTERVAL > 1: the interval-deformable ResNet is not supported")
    sc.mobilenet = int(bool(m.get("MOBILENET", False)))  # MobileNetV2 bottom-up (csrc/conv_dw.hip): MODEL.RESNETS.* is not read
    sc.resnet_depth = int(m.RESNETS.DEPTH)
    sc.stride_in_1x1 = int(bool(m.RESNETS.get("STRIDE_IN_1X1", True)))
    sc.num_cls_convs = int(f.NUM_CLS_CONVS)
    sc.num_box_convs = int(f.NUM_BOX_CONVS)
    sc.num_share_convs = int(f.NUM_SHARE_CONVS)
    # the last conv of the cls and of the bbox tower becomes adet's modulated deformable DFConv2d (fcos.py:83-84, 391-395)
    sc.tower_deformable = int(bool(f.get("USE_DEFORMABLE", False)))
    # backbone branches the five target configs leave at their defaults: refuse them instead of silently building the default graph
    r = m.RESNETS
    # ResNeXt (grouped 3x3 conv2, csrc/conv_group.hip): per-group width WIDTH_PER_GROUP << s a power of two in [4, 64] at every stage,
    # NUM_GROUPS * WIDTH_PER_GROUP a multiple of 64; the plain ResNet bottleneck is 1 group x 64
    ng, wpg = int(r.get("NUM_GROUPS", 1)), int(r.get("WIDTH_PER_GROUP", 64))
    # R-18 / R-34 (detectron2 BasicBlock, csrc/conv_rw64.hip): stage widths 64 << s, i.e. RES2_OUT_CHANNELS 64; STRIDE_IN_1X1 is ignored
    # (the stride sits on conv1).  detectron2's own assertions for these depths: no groups, no deformable stages, no res5 dilation
    basic = sc.resnet_depth in (18, 34)
    if sc.mobilenet:
        sc.resnet_depth, ng, wpg = 50, 1, 64  # (not read: the C side sees the defaults)
    elif sc.resnet_depth not in (18, 34, 50, 101, 152):
        raise NotImplementedError(f"MODEL.RESNETS.DEPTH {sc.resnet_depth}: 18, 34 (BasicBlock) and 50, 101, 152 (bottleneck) are supported")
    if not sc.mobilenet and (ng != 1 or wpg != 64):
        if sc.resnet_depth not in (50, 101, 152):
            raise NotImplementedError(f"MODEL.RESNETS.DEPTH {sc.resnet_depth}: ResNeXt needs DEPTH 50, 101 or 152")
        widths = [wpg << s for s in range(4)]
        if ng < 1 or wpg < 1 or any(w < 4 or w > 64 or (w & (w - 1)) for w in widths) or (ng * wpg) % 64 != 0:
            raise NotImplementedError(
                f"MODEL.RESNETS.NUM_GROUPS {ng} / WIDTH_PER_GROUP {wpg}: the grouped conv needs a per-group width WIDTH_PER_GROUP << s "
                f"that is a power of two in [4, 64] at every stage (here {widths}) and NUM_GROUPS * WIDTH_PER_GROUP a multiple of 64")
    sc.num_groups, sc.width_per_group = ng, wpg
    if not sc.mobilenet:
        _check_resnet_keys(sc, r, basic)
    fpn = m.get("FPN", None)
    if fpn is not None:
        if str(fpn.get("FUSE_TYPE", "sum")) != "sum":
            raise NotImplementedError(f"MODEL.FPN.FUSE_TYPE {fpn.FUSE_TYPE!r}: only 'sum' is supported")
        if str(fpn.get("NORM", "") or "") != "":
            raise NotImplementedError(f"MODEL.FPN.NORM {fpn.NORM!r}: only '' (bias convs) is supported")
        if int(fpn.get("OUT_CHANNELS", 256)) != 256:
            raise NotImplementedError("MODEL.FPN.OUT_CHANNELS: only 256 is supported")
    norm = "" if f.NORM is None else str(f.NORM)
    if norm in ("GN", "NaiveGN"):  # adet's NaiveGroupNorm computes GroupNorm(32, C) by hand: the same arithmetic
        sc.tower_norm = 0
    elif norm in ("none", ""):     # fcos.py:399: "none" -> no norm layer: conv + ReLU towers
        sc.tower_norm = 1
    else:
        raise NotImplementedError(f"MODEL.FCOS.NORM {norm!r}: 'GN', 'NaiveGN' and 'none' are supported (the per-level BatchNorm variants are not)")
    strides = list(f.FPN_STRIDES)
    sc.nlevels = len(strides)
    for i, s in enumerate(strides):
        sc.strides[i] = int(s)
    for i in range(3):
        sc.pixel_mean[i] = float(m.PIXEL_MEAN[i])
        sc.pixel_std[i] = float(m.PIXEL_STD[i])
    sc.use_scale = int(bool(f.USE_SCALE))
    sc.pre_nms_thresh = float(f.INFERENCE_TH_TEST)
    sc.pre_nms_topk = int(f.PRE_NMS_TOPK_TEST)
    sc.nms_thresh = float(f.NMS_TH)
    sc.post_nms_topk = int(f.POST_NMS_TOPK_TEST)
    # fcos_outputs.py:937 `if self.thresh_with_ctr or OWD` / :951 `if not self.thresh_with_ctr and not OWD`: with OWD the all-ones class
    # is multiplied by the box quality BEFORE the threshold test, i.e. OWD decodes exactly like THRESH_WITH_CTR (round 5; round 4
    # thresholded the constant 1 and kept every location as a candidate)
    sc.thresh_with_ctr = int(bool(f.THRESH_WITH_CTR) or bool(m.PROPOSAL_GENERATOR.get("OWD", False)))
    bq = sorted(list(f.BOX_QUALITY))
    if bq == ["ctrness"]:
        sc.quality_mode = 0
    elif bq == ["iou"]:
        sc.quality_mode = 1
    elif bq == ["ctrness", "iou"]:
        sc.quality_mode = 2
    else:
        raise NotImplementedError(f"MODEL.FCOS.BOX_QUALITY {bq}")
    sc.prior_prob = float(f.PRIOR_PROB)
    if not bool(m.META_LEARN.EPISODIC_LEARNING):
        # plain base detector (meta_one_stage_detector.py:52-58: no code generator is built): the head runs the checkpoint's
        # own 1x1 cls_logits through the class-conditional conv, always with its bias
        if int(f.get("CLS_LOGITS_KERNEL_SIZE", 3)) not in (1, 3):
            raise NotImplementedError("base-detector inference needs MODEL.FCOS.CLS_LOGITS_KERNEL_SIZE 1 or 3")
        sc.cond_use_bias = 1
        return sc
    cg = m.META_LEARN.CODE_GENERATOR
    # knobs that change the reference arithmetic and are not implemented must fail loudly, not be ignored
    if bool(cg.ROI_BOX.get("FPN_MULTILEVEL_FEATURE", False)):
        # the reference cannot run it either: CodeGeneratorHead builds detectron2's ROIPooler (one output tensor), code_generator.py:943
        # then iterates over its batch dimension and GroupNorm fails on the unbatched slices
        raise NotImplementedError("CODE_GENERATOR.ROI_BOX.FPN_MULTILEVEL_FEATURE is not supported (it fails in the reference too)")
    # (USE_PER_CLS_SCALE is set by the LVIS yamls but never read by the reference; INIT_NORM_LAYER only affects initialisation)
    for knob in ("ALL_MASK", "USE_DEFORMABLE", "META_WEIGHT"):
        if bool(cg.get(knob, False)):
            raise NotImplementedError(f"CODE_GENERATOR.{knob} is not supported")
    if str(cg.ROI_BOX.get("POOLER_TYPE", "ROIAlignV2")) != "ROIAlignV2":
        raise NotImplementedError("CODE_GENERATOR.ROI_BOX.POOLER_TYPE must be ROIAlignV2")
    sc.cg_meta_bias = int(bool(cg.get("META_BIAS", False)))
    sc.cond_use_bias = int(bool(cg.USE_BIAS))
    cg_name = str(cg.NAME)
    if cg_name not in ("CodeGenerator", "ROIEncoder"):
        # a plugged-in component (modeling.CODE_GENERATOR_REGISTRY) names the in-library generator it drives
        from .modeling import CODE_GENERATOR_REGISTRY
        comp = CODE_GENERATOR_REGISTRY.get(cg_name) if cg_name in CODE_GENERATOR_REGISTRY else None
        cg_name = getattr(comp, "engine_generator", None) or cg_name
    if cg_name == "ROIEncoder":
        # sylph/modeling/code_generator/roi_encoder.py:206-281 (dims of the LVIS ROI-Encoder yaml)
        sc.cg_type = 1
        tk, te, hd = cg.TOKENIZER, cg.TRANSFORMER_ENCODER, cg.HEAD
        if int(tk.CONV_DIM) != 256 or int(tk.FC_DIM) != 256 or int(hd.OUTPUT_DIM) != 256:
            raise NotImplementedError("ROIEncoder: TOKENIZER.CONV_DIM / FC_DIM and HEAD.OUTPUT_DIM must be 256")
        if int(tk.NUM_CONV) > 0 and str(tk.NORM) != "GN":
            raise NotImplementedError("ROIEncoder: TOKENIZER.NORM must be 'GN'")
        if int(cg.ROI_BOX.POOLER_RESOLUTION) != 7:
            raise NotImplementedError("ROI_BOX.POOLER_RESOLUTION must be 7")
        sc.tok_num_conv, sc.tok_num_fc = int(tk.NUM_CONV), int(tk.NUM_FC)
        sc.enc_layers, sc.head_num_fc, sc.head_fc_dim = int(te.LAYERS), int(hd.NUM_FC), int(hd.FC_DIM)
        sc.cond_use_bias = 1  # CondConvBlock always passes the bias (head_utils.py:140-162)
        return sc
    if cg_name != "CodeGenerator":
        raise NotImplementedError(f"{cg.NAME} is not implemented")
    tl = list(cg.TOWER_LAYERS)
    sc.cg_tower_layers = len(tl)
    sc.cg_tower_gn_mask = sc.cg_tower_relu_mask = 0
    for i, layer in enumerate(tl):  # [norm, activation] (code_generator.py:648-688)
        norm, act = (list(layer) + ["", ""])[:2]
        norm, act = ("" if norm is None else str(norm)), ("" if act is None else str(act))
        if norm in ("GN", "NaiveGN"):
            sc.cg_tower_gn_mask |= 1 << i
        elif norm not in ("", "none"):
            raise NotImplementedError(f"CODE_GENERATOR.TOWER_LAYERS entry {layer}: norm must be 'GN' or '' (LN / BN / IN are not supported)")
        if act == "ReLU":
            sc.cg_tower_relu_mask |= 1 << i
        elif act != "":  # the reference builds nothing for other strings except "Tanh"
            raise NotImplementedError(f"CODE_GENERATOR.TOWER_LAYERS entry {layer}: activation must be 'ReLU' or ''")
    if len(tl) > 30:
        raise NotImplementedError("more than 30 CODE_GENERATOR.TOWER_LAYERS")
    # CLS_LAYER = [norm, activation, k]: k is the spatial size of the class code (GlobalAdaptiveAvgPool2d(k_s = k), code_generator.py:
    # 519-540), run by the query head as a k x k conv with padding k // 2 (fcos.py:499-510).  2 cannot run in the reference (padding 1
    # with an even kernel grows the map); larger sizes are not implemented
    cl = list(cg.CLS_LAYER)
    if len(cl) != 3 or cl[0] not in ("", "none") or cl[1] != "" or int(cl[2]) not in (1, 3):
        raise NotImplementedError(f"CODE_GENERATOR.CLS_LAYER {cl} (only ['', '', 1] and ['', '', 3]: no norm, no activation, a 1x1 or 3x3 class code)")
    sc.cg_code_ksize = int(cl[2])
    if sc.cg_code_ksize == 3 and sc.tower_deformable and sc.tower_norm == 0 and _env_int("SYLPH_GN_COND3X3", 0):
        # gn_cond3x3_kernel adds nine per-tap accumulators, the default route (GroupNorm apply + conv_igemm) one: scores one fp32 ulp
        # apart, where deformable towers promise the default route's detections bit for bit.  sylph_fcos_head refuses it per call too
        # (the variable is read at every head call)
        raise NotImplementedError("SYLPH_GN_COND3X3=1 with MODEL.FCOS.USE_DEFORMABLE: the fused 3x3 class-code route is not offered for "
                                  "deformable towers (its scores differ from the default route's in the last fp32 bit); unset SYLPH_GN_COND3X3")
    bl = list(cg.BIAS_LAYER)
    sc.cg_has_bias = int(len(bl) != 0)
    if len(bl) and (len(bl) != 3 or bl[0] not in ("", "none") or bl[1] != "" or int(bl[2]) != 1):
        raise NotImplementedError(f"CODE_GENERATOR.BIAS_LAYER {bl} (only [] or ['', '', 1]: no norm, no ReLU, one conv)")
    for knob, field in (("WEIGHT_LAYER", "cg_has_weight"), ("SCALE_LAYER", "cg_has_scale")):
        lay = list(cg.get(knob, []))
        # [norm, relu, pool]: a 1-channel 3x3 conv + global average pool (code_generator.py:583-645); a norm layer on one channel
        # cannot be built by the reference either (GroupNorm(32, 1)), the other two entries are not read
        if len(lay) and (len(lay) != 3 or lay[0] not in ("", "none")):
            raise NotImplementedError(f"CODE_GENERATOR.{knob} {lay} (only [] or ['', '', 1])")
        setattr(sc, field, int(len(lay) != 0))
    if bool(cg.COMPRESS_CODE_W_MAX) or bool(cg.CLS_REWEIGHT) or bool(cg.BOX_ON):
        raise NotImplementedError("COMPRESS_CODE_W_MAX / CLS_REWEIGHT / BOX_ON are not supported")
    sc.cg_bias_l2_norm = int(bool(cg.BIAS_L2_NORM))
    sc.cg_post_norm = int(str(cg.POST_NORM) != "")
    if sc.cg_post_norm and str(cg.POST_NORM) != "GN":
        raise NotImplementedError("CODE_GENERATOR.POST_NORM must be '' or 'GN'")
    sc.cg_conv_l2_norm = int(bool(cg.CONV_L2_NORM))
    sc.cg_use_weight_scale = int(bool(cg.USE_WEIGHT_SCALE))
    return sc


def code_set_offsets(n_classes: Sequence[int]) -> List[int]:
    """First row of every code set in the (sum N, 256) table of `Engine.head_code_sets` -- and first channel of its logits in what
    `export_head` returns afterwards -- followed by sum N: [0, N_0, N_0 + N_1, ..., sum N]."""
    off = [0]
    for g, n in enumerate(n_classes):
        if int(n) < 1:
            raise ValueError(f"code set {g} is empty (N_g = {int(n)}): every set needs at least one class")
        off.append(off[-1] + int(n))
    return off


def check_code_sets(codes, code_ksize: int = 1) -> List[int]:
    """Validate the `[(cls_conv, cls_bias), ...]` argument of `Engine.head_code_sets` (no GPU needed) -> classes per set."""
    if code_ksize != 1:
        raise NotImplementedError(f"head_code_sets runs 1x1 class codes only: CODE_GENERATOR.CLS_LAYER kernel size {code_ksize} is not "
                                  "supported here (call head once per code set)")
    codes = list(codes)
    if len(codes) == 0:
        raise ValueError("head_code_sets needs at least one code set (G = 0)")
    n = []
    for g, (w, b) in enumerate(codes):
        if w.dim() != 4:
            raise ValueError(f"code set {g}: Weight has dimension: {w.dim()}")
        if w.size(2) != 1 or w.size(3) != 1:
            raise ValueError(f"code set {g}: class code of spatial size {w.size(2)}x{w.size(3)}: cls_conv must be (N, 256 k, 1, 1)")
        if w.size(1) < 256 or w.size(1) % 256 != 0:
            raise ValueError(f"code set {g}: weight has wrong shape, {tuple(w.shape)}: 256 channels (or a multiple, ROIEncoder) expected")
        if b is not None and b.numel() != w.size(0):
            raise ValueError(f"code set {g}: {b.numel()} biases for {w.size(0)} classes")
        n.append(int(w.size(0)))
    code_set_offsets(n)  # (an empty set)
    if len({b is None for _, b in codes}) != 1:
        raise ValueError("cls_bias must be given for every code set or for none")
    return n


class QueryRecord:
    """What the towers left for one batch (sylph_record_store): an immutable device snapshot that any head entry can score, any number of
    times, without the backbone and the towers (Engine.load_record).  Owned by the caller; `close()` gives its bytes back."""

    def __init__(self, engine: "Engine", handle: c_void_p, sizes: List[Tuple[int, int]]):
        self._engine = engine
        self._h = handle
        B, H, W, n = c_int(0), c_int(0), c_int(0), c_int64(0)
        check(engine.L.sylph_record_info(handle, ctypes.byref(B), ctypes.byref(H), ctypes.byref(W), ctypes.byref(n)), "record_info")
        self.batch = (B.value, H.value, W.value, list(sizes))  # (B, padded H, padded W, [(h, w) per image]), as Engine._batch
        self.nbytes = int(n.value)

    @property
    def closed(self) -> bool:
        return self._h is None

    def close(self):
        if self._h is not None:
            eng, h = self._engine, self._h
            self._h = None
            if eng._ctx:  # (a closed engine has released its records already)
                eng.L.sylph_record_destroy(eng._ctx, h)
                if eng._record is self:
                    eng._record = None
                    eng._batch = None
            if self in eng._records:
                eng._records.remove(self)


class BoxSamples:
    """A box-sample bank (Engine.box_samples): what the trainable box branch reads of the positive locations of one or more batches.
    patches (n, 3, 3, 256) bf16: the normalised bbox tower output at the nine taps; targets (n, 4) fp32: (l, t, r, b) / stride;
    info (n, 4) int32: (row, level, box index, class).  Device tensors; `count` is the number of positives found (above n only after an
    overflow of the capacity)."""

    def __init__(self, patches: torch.Tensor, targets: torch.Tensor, info: torch.Tensor, count: Optional[int] = None, overflow: bool = False):
        self.patches, self.targets, self.info = patches, targets, info
        self.n = int(info.shape[0])
        self.count = self.n if count is None else int(count)
        self.overflow = bool(overflow)

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.patches, self.targets, self.info))

    @staticmethod
    def cat(banks: Sequence["BoxSamples"]) -> "BoxSamples":
        """the banks of several batches as one, in the order given (rows and box indices stay those of their own batch)"""
        banks = list(banks)
        if not banks:
            raise ValueError("BoxSamples.cat: no banks")
        return BoxSamples(torch.cat([b.patches for b in banks]).contiguous(), torch.cat([b.targets for b in banks]).contiguous(),
                          torch.cat([b.info for b in banks]).contiguous())

    def select(self, index: torch.Tensor) -> "BoxSamples":
        """the samples `index` (a device index tensor) as a bank of their own"""
        return BoxSamples(self.patches[index].contiguous(), self.targets[index].contiguous(), self.info[index].contiguous())


class Engine:
    """One HIP context: weights + per-batch-shape workspaces, all on ``device``."""

    def __init__(self, cfg=None, dtype: str = "bf16", device: int = 0, cand_cap: int = 0):
        if not torch.cuda.is_available():
            raise RuntimeError("sylph_amd.Engine needs a ROCm GPU (torch.cuda.is_available() is False); "
                               "there is no CPU fallback")
        self.L = _lib.lib()
        self.device = torch.device("cuda", device)
        self.dtype = dtype
        self._ctx = c_void_p(0)
        dt = {"bf16": _lib.SYLPH_BF16, "f32": _lib.SYLPH_F32, "fp32": _lib.SYLPH_F32, "f32s": _lib.SYLPH_F32S}[dtype]
        check(self.L.sylph_ctx_create(device, dt, ctypes.byref(self._ctx)), "ctx_create")
        self.sc = config_from_cfg(cfg)
        if cand_cap:
            self.sc.cand_cap = cand_cap
        check(self.L.sylph_set_config(self._ctx, ctypes.byref(self.sc)), "set_config")
        self.nlevels = self.sc.nlevels
        self.is_roi_encoder = int(self.sc.cg_type) == 1
        # CODE_GENERATOR.CLS_LAYER kernel size: a class code is (256, k, k), a packed code row 256 k^2 + 1 floats (the ROIEncoder's stay 1x1)
        self.code_ksize = 1 if self.is_roi_encoder else max(1, int(self.sc.cg_code_ksize))  # (0: a library build that predates the field, tools/ab_bench.sh)
        self.code_len = 256 * self.code_ksize ** 2 + 1
        self.cond_scale = 1.0  # CondConvBlock Scale of the first chunk (ROIEncoder head), read from the checkpoint
        self.cond_scales = [1.0]  # all CondConvBlock Scales (one per 256-channel chunk of the class code)
        self._cond_scales_loaded = False  # did the checkpoint carry cond_cls_logits.scales.*?
        # MODEL.PROPOSAL_GENERATOR.OWD (fcos_outputs.py:913-916): class probabilities are replaced by ONE all-ones class
        self.owd = bool(cfg.MODEL.PROPOSAL_GENERATOR.get("OWD", False)) if cfg is not None else False
        self._batch = None  # (B, H, W, [(h,w)...])
        self._sup_rows = None  # boxes of the last codegen* call: the rows of export_support's per-shot stages
        self._ncls = 0
        self._keep = []  # tensors that must outlive queued kernels
        self._lib_writes = 0  # in-place writes into caller tensors through raw pointers (part of the class-code cache key)
        self._records = []  # live QueryRecords of this engine
        self._record = None  # the one that is the current batch (load_record), None on a fresh batch
        self._merge_ws = None  # merge_views_large's workspace: grows on demand, contents are scratch
        self._ft_ws = None  # cls_grad's workspace (the per-unit partial sums): grows on demand, contents are scratch
        self._box_ws = None  # box_grad's workspace, likewise
        self._cgt_ws = None  # the generator's training workspace: the saved activations of a forward until its backward, then scratch
        # what the training-side entries (fcos_targets, cls_grad) read from MODEL.FCOS: focal loss and target assignment
        f = cfg.MODEL.FCOS if cfg is not None else {}
        self.fcos_train = {"alpha": float(f.get("LOSS_ALPHA", 0.25)), "gamma": float(f.get("LOSS_GAMMA", 2.0)),
                           "sizes_of_interest": [float(v) for v in f.get("SIZES_OF_INTEREST", [64, 128, 256, 512])],
                           "center_sample": bool(f.get("CENTER_SAMPLE", True)), "pos_radius": float(f.get("POS_RADIUS", 1.5)),
                           "prior_prob": float(f.get("PRIOR_PROB", 0.01)),
                           # ... and the box losses (box_samples, box_grad)
                           "box_quality": [str(v) for v in f.get("BOX_QUALITY", ["ctrness"])], "iou_mask": bool(f.get("IOU_MASK", False)),
                           "loc_loss_type": str(f.get("LOC_LOSS_TYPE", "giou"))}
        self._counts_free = {}  # length -> pinned count buffers no handle owns (_counts_acquire)
        self._counts_out = set()  # ids of the pinned count buffers that unfetched decode handles own

    def close(self):
        if self._ctx:
            for rec in list(getattr(self, "_records", [])):
                rec.close()
            self.L.sylph_ctx_destroy(self._ctx)
            self._ctx = c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        check(self.L.sylph_set_stream(self._ctx, c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    # ---- weights ------------------------------------------------------------------------------
    def load_state_dict(self, sd: Dict[str, torch.Tensor]):
        """Reference checkpoint keys -> packed device weights."""
        for k, v in sd.items():
            if not torch.is_tensor(v) or not v.is_floating_point():
                continue
            if ".fcos_head.cond_cls_logits.scales." in k and k.endswith(".scale"):
                i = int(k.split(".scales.")[1].split(".")[0])
                while len(self.cond_scales) <= i:
                    self.cond_scales.append(1.0)
                self.cond_scales[i] = float(v.reshape(-1)[0])
                self._cond_scales_loaded = True
                if i == 0:
                    self.cond_scale = self.cond_scales[0]
            t = v.detach().to("cpu", torch.float32).contiguous()
            shape = (c_int64 * max(t.dim(), 1))(*(list(t.shape) if t.dim() else [1]))
            check(self.L.sylph_load_weight(self._ctx, k.encode(), c_void_p(t.data_ptr()), shape, max(t.dim(), 1)),
                  f"load_weight({k})")
        check(self.L.sylph_finalize_weights(self._ctx), "finalize_weights")
        self._codes_key = None  # packed class codes depend on the checkpoint's CondConvBlock scales: never reuse across a reload

    # ---- query / support image path ----------------------------------------------------------------
    def level_shapes(self, H: int, W: int) -> List[Tuple[int, int]]:
        h, w = H // 8, W // 8
        out = []
        for _ in range(self.nlevels):
            out.append((h, w))
            h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        return out

    def preprocess(self, images: List[torch.Tensor]) -> Tuple[int, int]:
        self._stream()
        imgs = [im.to(self.device, torch.float32).contiguous() for im in images]
        B = len(imgs)
        ptrs = (c_void_p * B)(*[im.data_ptr() for im in imgs])
        hs, ws = _iarr([im.shape[1] for im in imgs]), _iarr([im.shape[2] for im in imgs])
        ph, pw = c_int(0), c_int(0)
        check(self.L.sylph_preprocess(self._ctx, B, ptrs, hs, ws, ctypes.byref(ph), ctypes.byref(pw)), "preprocess")
        self._keep = imgs
        self._batch = (B, ph.value, pw.value, [(int(im.shape[1]), int(im.shape[2])) for im in imgs])
        self._record = None
        return ph.value, pw.value

    def preprocess_u8(self, images: List[torch.Tensor], new_sizes: List[Tuple[int, int]], rgb_input: bool = False) -> Tuple[int, int]:
        """Fused input pipeline: (h, w, 3) uint8 HWC images (device, or pinned host: copied asynchronously here) ->
        PIL-exact BILINEAR resize to new_sizes -> BGR -> normalise -> pad; one kernel (sylph_preprocess_u8)."""
        self._stream()
        imgs = [im.to(self.device, non_blocking=True).contiguous() for im in images]
        for im in imgs:
            assert im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3, "uint8 HWC images expected"
        B = len(imgs)
        ptrs = (c_void_p * B)(*[im.data_ptr() for im in imgs])
        ph, pw = c_int(0), c_int(0)
        check(self.L.sylph_preprocess_u8(self._ctx, B, ptrs, _iarr([im.shape[0] for im in imgs]), _iarr([im.shape[1] for im in imgs]),
                                         _iarr([s[0] for s in new_sizes]), _iarr([s[1] for s in new_sizes]), int(rgb_input),
                                         ctypes.byref(ph), ctypes.byref(pw)), "preprocess_u8")
        self._keep = imgs
        self._batch = (B, ph.value, pw.value, [(int(s[0]), int(s[1])) for s in new_sizes])
        self._record = None
        return ph.value, pw.value

    def preprocess_views(self, sources: List[torch.Tensor], views: List[Dict], rgb_input: bool = False) -> Tuple[int, int]:
        """The input pipeline for VIEWS of resident sources (sylph_preprocess_views): `sources` are (h, w, 3) uint8 HWC images (device,
        or pinned host: each is copied once, however many views name it), `views` dicts {"source": index into sources, "crop": (x0, y0,
        cw, ch), "size": (new_h, new_w), "flip": bool} (sylph_amd.views).  Image b of the batch is crop -> PIL-exact BILINEAR resize ->
        mirror when flipped -> BGR -> normalise -> pad: what preprocess_u8 writes for a host-made copy of the view, in one kernel."""
        self._stream()
        srcs = [im.to(self.device, non_blocking=True).contiguous() for im in sources]
        for im in srcs:
            assert im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3, "uint8 HWC images expected"
        B = len(views)
        vs = [srcs[int(v["source"])] for v in views]
        ptrs = (c_void_p * B)(*[im.data_ptr() for im in vs])
        crops = [[int(t) for t in v["crop"]] for v in views]
        sizes = [(int(v["size"][0]), int(v["size"][1])) for v in views]
        ph, pw = c_int(0), c_int(0)
        check(self.L.sylph_preprocess_views(self._ctx, B, ptrs, _iarr([im.shape[0] for im in vs]), _iarr([im.shape[1] for im in vs]),
                                            _iarr([c[0] for c in crops]), _iarr([c[1] for c in crops]), _iarr([c[2] for c in crops]),
                                            _iarr([c[3] for c in crops]), _iarr([s[0] for s in sizes]), _iarr([s[1] for s in sizes]),
                                            _iarr([1 if v.get("flip", False) else 0 for v in views]), int(rgb_input),
                                            ctypes.byref(ph), ctypes.byref(pw)), "preprocess_views")
        self._keep = srcs
        self._batch = (B, ph.value, pw.value, sizes)
        self._record = None
        return ph.value, pw.value

    def export_input(self) -> torch.Tensor:
        self._stream()
        B, H, W, _ = self._batch
        out = torch.empty(B, 3, H, W, device=self.device)
        check(self.L.sylph_export_input(self._ctx, _ptr(out)), "export_input")
        return out

    def backbone(self):
        self._stream()
        check(self.L.sylph_backbone_fpn(self._ctx), "backbone_fpn")

    def import_pyramid(self, levels: List[torch.Tensor], padded_hw: Tuple[int, int],
                       image_sizes: Optional[List[Tuple[int, int]]] = None):
        self._stream()
        B = levels[0].shape[0]
        H, W = padded_hw
        lv = [t.to(self.device, torch.float32).contiguous() for t in levels]
        exp = self.level_shapes(H, W)
        for t, (h, w) in zip(lv, exp):
            assert tuple(t.shape) == (B, 256, h, w), f"level shape {tuple(t.shape)} != {(B, 256, h, w)}"
        sizes = image_sizes or [(H, W)] * B
        ptrs = (c_void_p * len(lv))(*[t.data_ptr() for t in lv])
        check(self.L.sylph_import_pyramid(self._ctx, B, H, W, _iarr([s[0] for s in sizes]),
                                          _iarr([s[1] for s in sizes]), ptrs), "import_pyramid")
        self._keep = lv
        self._batch = (B, H, W, list(sizes))
        self._record = None

    def export_pyramid(self) -> List[torch.Tensor]:
        self._stream()
        B, H, W, _ = self._batch
        out = []
        for l, (h, w) in enumerate(self.level_shapes(H, W)):
            t = torch.empty(B, 256, h, w, device=self.device, dtype=torch.float32)
            check(self.L.sylph_export_pyramid(self._ctx, l, _ptr(t)), "export_pyramid")
            out.append(t)
        return out

    # ---- query records: the towers once, class codes any number of times ------------------------------------------
    def towers(self):
        """The class-agnostic part of the head (towers, box / centerness / IoU predictions, cls GroupNorm statistics) on the current fresh
        batch, with no class codes: what `store_record` snapshots.  Leaves nothing to decode."""
        self._stream()
        check(self.L.sylph_fcos_towers(self._ctx), "fcos_towers")
        self._ncls = 0

    def store_record(self) -> QueryRecord:
        """Snapshot of what the towers left for the current fresh batch (after `towers()` or any head call on it)."""
        self._stream()
        if getattr(self, "_batch", None) is None:
            raise RuntimeError("store_record: no current batch")
        h = c_void_p(0)
        check(self.L.sylph_record_store(self._ctx, ctypes.byref(h)), "record_store")
        rec = QueryRecord(self, h, self._batch[3])
        self._records.append(rec)
        return rec

    def load_record(self, rec: QueryRecord):
        """Make `rec` the current batch: head*, decode* and export_head then work as on the fresh batch, without running the towers."""
        if not isinstance(rec, QueryRecord):
            raise TypeError(f"load_record: a QueryRecord is expected, not {type(rec).__name__}")
        if rec.closed:
            raise RuntimeError("load_record: the query record is closed")
        self._stream()
        check(self.L.sylph_record_load(self._ctx, rec._h), "record_load")
        self._batch = rec.batch
        self._record = rec
        self._keep = []
        self._ncls = 0

    # ---- fine-tuning the class codes on the current batch's tower outputs (sylph_amd.finetune) ---------------------------------
    def batch_rows(self) -> int:
        """Rows of the current batch's tower output: B x the locations of the padded pyramid."""
        if getattr(self, "_batch", None) is None:
            raise RuntimeError("no current batch")
        B, H, W, _ = self._batch
        return B * sum(h * w for h, w in self.level_shapes(H, W))

    def _check_gt(self, who: str, boxes, classes, image_index):
        """The ground truth of the current batch validated on the host, under the entry's name: one class and one image per box,
        image_index sorted and inside the batch -> (boxes (n, 4) fp32, classes (n,) int32, image_index (n,) int32) on the device."""
        bx = torch.as_tensor(boxes, dtype=torch.float32).reshape(-1, 4)
        cl = torch.as_tensor(classes).reshape(-1)
        im = torch.as_tensor(image_index).reshape(-1)
        n = bx.shape[0]
        if cl.numel() != n or im.numel() != n:
            raise ValueError(f"{who}: {n} boxes, {cl.numel()} classes and {im.numel()} image indices")
        B = self._batch[0]
        iml = im.tolist()
        if any(a > b for a, b in zip(iml, iml[1:])):
            raise ValueError(f"{who}: gt_image is not sorted (image_index must not decrease)")
        if n and (iml[0] < 0 or iml[-1] >= B):
            raise ValueError(f"{who}: image_index outside the batch of {B} images")
        return bx.to(self.device).contiguous(), cl.to(self.device, torch.int32).contiguous(), im.to(self.device, torch.int32).contiguous()

    def _grow_ws(self, attr: str, need: int) -> torch.Tensor:
        """The engine's scratch workspace `attr` with room for `need` bytes: it grows on demand and is never empty."""
        ws = getattr(self, attr)
        if ws is None or ws.numel() < need:
            ws = torch.empty(max(need, 4), device=self.device, dtype=torch.uint8)
            setattr(self, attr, ws)
        return ws

    def fcos_targets(self, boxes: torch.Tensor, classes: torch.Tensor, image_index: torch.Tensor):
        """FCOS classification targets of the current batch (a fresh batch after `towers()`, or a loaded record): `boxes` (n, 4) in
        network-input pixels, `classes` (n,), `image_index` (n,) sorted.  Returns (labels, num_pos): int32 device tensors, one label per
        row of the tower output (-1: background) and the count of positives; nothing is read back.  (The arguments are validated on
        the host: device tensors are copied back for that.)"""
        self._stream()
        rows = self.batch_rows()
        bx, cl, im = self._check_gt("fcos_targets", boxes, classes, image_index)
        n = bx.shape[0]
        if n and int(torch.as_tensor(classes).min()) < 0:
            raise ValueError("fcos_targets: a class index is negative")
        fc = self.fcos_train
        labels = torch.empty(rows, device=self.device, dtype=torch.int32)
        num_pos = torch.empty(1, device=self.device, dtype=torch.int32)
        soi = (ctypes.c_float * len(fc["sizes_of_interest"]))(*fc["sizes_of_interest"])
        check(self.L.sylph_fcos_targets(self._ctx, n, _ptr(bx), _ptr(cl), _ptr(im), soi, len(fc["sizes_of_interest"]),
                                        int(fc["center_sample"]), float(fc["pos_radius"]), _ptr(labels), _ptr(num_pos)), "fcos_targets")
        return labels, num_pos

    def cls_grad(self, labels: torch.Tensor, cls_conv: torch.Tensor, cls_bias: Optional[torch.Tensor], class_offset: int = 0,
                 check_labels: bool = True):
        """Sum of the sigmoid focal loss over the current batch's locations and the N classes of `cls_conv` (N, 256[, 1, 1]), and its
        gradient: (loss_sum (1,), grad_w (N, 256), grad_b (N,) or None), fp32 device tensors, not divided by the number of positives.
        Class n is label class_offset + n.  check_labels reads the largest label back (one sync) and refuses a label >= N by name; a
        loop that has validated its annotations passes False."""
        self._stream()
        if not torch.is_tensor(labels) or labels.dtype != torch.int32 or labels.device != self.device or labels.numel() != self.batch_rows():
            raise ValueError(f"cls_grad: labels must be the int32 device tensor of {self.batch_rows()} rows fcos_targets returns for this batch")
        w = cls_conv.to(self.device, torch.float32).reshape(cls_conv.shape[0], -1).contiguous()
        if w.shape[1] != 256:
            raise ValueError(f"cls_grad: 3x3 class codes are not supported: cls_conv must be (N, 256) or (N, 256, 1, 1), not {tuple(cls_conv.shape)}")
        N = w.shape[0]
        b = cls_bias.to(self.device, torch.float32).reshape(-1).contiguous() if cls_bias is not None else None
        if b is not None and b.numel() != N:
            raise ValueError(f"cls_grad: {b.numel()} biases for {N} classes")
        if check_labels and class_offset == 0 and labels.numel() and int(labels.max()) >= N:
            raise ValueError(f"cls_grad: a label >= N (largest label {int(labels.max())}, {N} classes)")
        need = c_int64(0)
        check(self.L.sylph_cls_grad_bytes(self._ctx, N, ctypes.byref(need)), "cls_grad_bytes")
        ws = self._grow_ws("_ft_ws", need.value)
        loss = torch.empty(1, device=self.device, dtype=torch.float32)
        gw = torch.empty(N, 256, device=self.device, dtype=torch.float32)
        gb = torch.empty(N, device=self.device, dtype=torch.float32) if b is not None else None
        fc = self.fcos_train
        check(self.L.sylph_cls_grad(self._ctx, _ptr(labels), _ptr(w), _ptr(b), N, int(class_offset), float(fc["alpha"]), float(fc["gamma"]),
                                    _ptr(ws), _ptr(loss), _ptr(gw), _ptr(gb)), "cls_grad")
        self._keep_ft = (w, b)
        return loss, gw, gb

    # ---- fine-tuning the box branch on a bank of positive samples (sylph_amd.finetune.finetune_box_branch) ----------------------
    def _box_refuse(self, who: str):
        from .finetune import _single_rank
        _single_rank(who)
        fc = self.fcos_train
        if fc["loc_loss_type"] != "giou":
            raise NotImplementedError(f"{who}: MODEL.FCOS.LOC_LOSS_TYPE \"{fc['loc_loss_type']}\" is not supported (the gradient kernel implements \"giou\")")

    def box_samples(self, boxes: torch.Tensor, classes: torch.Tensor, image_index: torch.Tensor, max_samples: Optional[int] = None,
                    out=None, allow_overflow: bool = False) -> "BoxSamples":
        """The box-sample bank of the current FRESH batch (after `towers()` or a head call): one sample per positive location of
        `fcos_targets`' assignment, in ascending row order.  Arguments as `fcos_targets`.  max_samples: the capacity (default: a bound that
        cannot overflow: 9 per box and level under centre sampling with POS_RADIUS <= 1.5, else every row); a count above it raises unless
        allow_overflow (then `.overflow` is set and `.count` is the true count).  out: (patches, targets, info) tensors of at least
        max_samples rows to write into.  Reads the count back (one sync)."""
        self._stream()
        self._box_refuse("box_samples")
        if getattr(self, "_batch", None) is None:
            raise RuntimeError("box_samples: no current batch")
        rows = self.batch_rows()
        bx, cl, im = self._check_gt("box_samples", boxes, classes, image_index)
        n = bx.shape[0]
        fc = self.fcos_train
        if max_samples is None:
            cap = rows if not (fc["center_sample"] and fc["pos_radius"] <= 1.5) else min(rows, 9 * self.nlevels * n)
        else:
            cap = int(max_samples)
            if cap < 0:
                raise ValueError("box_samples: max_samples is negative")
        if out is None:
            patches = torch.empty(cap, 3, 3, 256, device=self.device, dtype=torch.bfloat16)
            targets = torch.empty(cap, 4, device=self.device, dtype=torch.float32)
            info = torch.empty(cap, 4, device=self.device, dtype=torch.int32)
        else:
            patches, targets, info = out
            if (patches.dtype != torch.bfloat16 or targets.dtype != torch.float32 or info.dtype != torch.int32 or
                    patches.numel() < cap * 2304 or targets.numel() < cap * 4 or info.numel() < cap * 4 or
                    not (patches.is_contiguous() and targets.is_contiguous() and info.is_contiguous())):
                raise ValueError(f"box_samples: out must be contiguous (patches bf16, targets fp32, info int32) device tensors of at least {cap} rows")
        cs = torch.empty(2, device=self.device, dtype=torch.int32)  # count | status
        soi = (ctypes.c_float * len(fc["sizes_of_interest"]))(*fc["sizes_of_interest"])
        check(self.L.sylph_box_samples(self._ctx, n, _ptr(bx), _ptr(cl), _ptr(im), soi, len(fc["sizes_of_interest"]), int(fc["center_sample"]),
                                       float(fc["pos_radius"]), cap, _ptr(patches), _ptr(targets), _ptr(info), _ptr(cs), _ptr(cs[1:])), "box_samples")
        count, status = (int(v) for v in cs.tolist())
        if status and not allow_overflow:
            raise RuntimeError(f"box_samples: {count} positive locations exceed max_samples = {cap}")
        k = min(count, cap)
        return BoxSamples(patches[:k], targets[:k], info[:k], count=count, overflow=bool(status))

    def box_grad(self, samples: "BoxSamples", w: torch.Tensor, b: torch.Tensor, scales: torch.Tensor, debug: bool = False,
                 quality=None, iou_mask: Optional[bool] = None):
        """Un-normalised box losses over the bank and their gradient with respect to the box branch: w (Cout, 256, 3, 3), b (Cout,),
        scales (levels,).  -> dict: sums (4,) = [sum weight (1 - giou), centerness BCE sum, IoU BCE sum, sum of centerness targets],
        grad_w, grad_b, grad_scales; with debug also z and g, the (n, Cout) pre-activations and d loss / d z.  quality / iou_mask
        default to MODEL.FCOS.BOX_QUALITY / IOU_MASK.  Nothing is read back."""
        self._stream()
        self._box_refuse("box_grad")
        if not isinstance(samples, BoxSamples):
            raise TypeError(f"box_grad: a BoxSamples bank is expected, not {type(samples).__name__}")
        cout, L = self.box_branch_shape()[:2]
        w = torch.as_tensor(w).to(self.device, torch.float32).contiguous()
        b = torch.as_tensor(b).to(self.device, torch.float32).reshape(-1).contiguous()
        s = torch.as_tensor(scales).to(self.device, torch.float32).reshape(-1).contiguous()
        if tuple(w.shape) != (cout, 256, 3, 3) or b.numel() != cout or s.numel() != L:
            raise ValueError(f"box_grad: the box branch is w ({cout}, 256, 3, 3), b ({cout},), scales ({L},); got {tuple(w.shape)}, "
                             f"{tuple(b.shape)}, {tuple(s.shape)}")
        q = sorted(self.fcos_train["box_quality"] if quality is None else quality)
        if q not in (["ctrness"], ["iou"], ["ctrness", "iou"]):
            raise NotImplementedError(f"box_grad: MODEL.FCOS.BOX_QUALITY {q}")
        qbits = (1 if "ctrness" in q else 0) | (2 if "iou" in q else 0)
        mask = self.fcos_train["iou_mask"] if iou_mask is None else bool(iou_mask)
        n = samples.n
        need = c_int64(0)
        check(self.L.sylph_box_grad_bytes(self._ctx, n, ctypes.byref(need)), "box_grad_bytes")
        ws = self._grow_ws("_box_ws", need.value)
        out = {"sums": torch.empty(4, device=self.device), "grad_w": torch.empty_like(w), "grad_b": torch.empty_like(b),
               "grad_scales": torch.empty_like(s)}
        if debug:
            out["z"] = torch.empty(n, cout, device=self.device)
            out["g"] = torch.empty(n, cout, device=self.device)
        check(self.L.sylph_box_grad(self._ctx, n, _ptr(samples.patches), _ptr(samples.targets), _ptr(samples.info), _ptr(w), _ptr(b), _ptr(s),
                                    qbits, int(mask), _ptr(ws), _ptr(out["sums"]), _ptr(out["grad_w"]), _ptr(out["grad_b"]),
                                    _ptr(out["grad_scales"]), _ptr(out.get("z")), _ptr(out.get("g"))), "box_grad")
        self._keep_box = (w, b, s, samples)
        return out

    def box_branch_shape(self):
        """(Cout, levels, stamp) of the box branch the context runs; stamp 0: the checkpoint's tensors"""
        co, lv, st = c_int(0), c_int(0), ctypes.c_uint64(0)
        check(self.L.sylph_box_branch_shape(self._ctx, ctypes.byref(co), ctypes.byref(lv), ctypes.byref(st)), "box_branch_shape")
        return co.value, lv.value, st.value

    def box_branch(self):
        """The box branch the context runs, as the state dict names it (CPU fp32): bbox_pred.weight|bias, ctrness.weight|bias,
        iou_overlap.weight|bias (a 6-channel branch), scales.{l}.scale"""
        from .finetune import split_box_branch
        cout, L, _ = self.box_branch_shape()
        w, b, s = torch.empty(cout, 256, 3, 3), torch.empty(cout), torch.empty(L)
        fp = lambda t: ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_float))
        check(self.L.sylph_get_box_branch(self._ctx, fp(w), fp(b), fp(s)), "get_box_branch")
        return split_box_branch(w, b, s)

    def set_box_branch(self, branch):
        """Install `branch` (the dict `box_branch()` returns, or None for the checkpoint's): from the next batch on every step is
        bit-identical to an engine loaded with a state dict carrying it.  No batch is current afterwards; query records stored under
        another branch are refused by `load_record` until that branch is back."""
        self._stream()
        if branch is None:
            check(self.L.sylph_set_box_branch(self._ctx, None, None, None), "set_box_branch")
        else:
            from .finetune import stack_box_branch
            cout, L, _ = self.box_branch_shape()
            w, b, s = (t.detach().to("cpu", torch.float32).contiguous() for t in stack_box_branch(branch))
            if tuple(w.shape) != (cout, 256, 3, 3) or b.numel() != cout or s.numel() != L:
                raise ValueError(f"set_box_branch: the box branch is w ({cout}, 256, 3, 3), b ({cout},), scales ({L},); got {tuple(w.shape)}, "
                                 f"{tuple(b.shape)}, {tuple(s.shape)}")
            fp = lambda t: ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_float))
            check(self.L.sylph_set_box_branch(self._ctx, fp(w), fp(b), fp(s)), "set_box_branch")
        self._batch = None
        self._record = None
        self._sup_rows = None
        self._keep = []
        self._ncls = 0

    def reset_box_branch(self):
        self.set_box_branch(None)

    def _fold_codes(self, cls_conv: torch.Tensor, cls_bias: Optional[torch.Tensor], raw: bool = False):
        """One episode's class codes -> ((N, 256) fp32, (N,) fp32 or None) on the device, the CondConvBlock of a ROIEncoder model folded in."""
        k = cls_conv.size(1) // 256
        assert cls_conv.size(1) == 256 * k and k >= 1, f"weight has wrong shape, {tuple(cls_conv.shape)}"
        assert k == 1 or (self.is_roi_encoder and not raw), "feature.size(1) != weight.size(1)"  # CondConvBasic (head_utils.py:69)
        # (a 3x3 code keeps torch's (c, ky, kx) order per row: 256 * 9 floats; the library packs it tap-major)
        w = cls_conv.to(self.device, torch.float32).reshape(cls_conv.size(0), -1)
        b = cls_bias.to(self.device, torch.float32).reshape(-1).contiguous() if cls_bias is not None else None
        if self.is_roi_encoder and not raw:
            # CondConvBlock (head_utils.py:140-162): sum over 256-channel chunks of scale_i * conv(feature, w_i, bias); the
            # reference indexes the Scale of chunk i+1 with i (head_utils.py:157-161).  conv is linear in (w, bias), so
            # the block is ONE class-conditional conv with w_eff = sum_i s_i' w_i and bias_eff = (sum_i s_i') bias.
            if not self._cond_scales_loaded:
                sc = [1.0 / k] * k  # Scale init of the reference (head_utils.py:131-136): no learned value in the checkpoint
            else:
                if len(self.cond_scales) < max(k - 1, 1):
                    raise ValueError(f"the checkpoint has {len(self.cond_scales)} cond_cls_logits scales; a {256 * k}-channel class "
                                     f"code needs {max(k - 1, 1)}")
                sc = list(self.cond_scales)
            per_chunk = [sc[0]] + [sc[i] for i in range(k - 1)]
            w = sum(s_ * w[:, 256 * i:256 * (i + 1)] for i, s_ in enumerate(per_chunk))
            b = b * float(sum(per_chunk)) if b is not None else None
        w = w.contiguous()
        if b is not None:
            assert b.numel() == w.size(0)
        return w, b

    def head(self, cls_conv: torch.Tensor, cls_bias: Optional[torch.Tensor], raw: bool = False):
        """raw=True: plain `conv(cls_tower, w, b)` even on a ROIEncoder model -- the checkpoint's own cls_logits run without the
        CondConvBlock Scale (forward_base_train, fcos.py:544-570,592-593)."""
        self._stream()
        assert cls_conv.dim() == 4, f"Weight has dimension: {cls_conv.dim()}"
        k = self.code_ksize
        if cls_conv.size(2) != k or cls_conv.size(3) != k:
            raise ValueError(f"class code of spatial size {cls_conv.size(2)}x{cls_conv.size(3)} on an engine configured for {k}x{k} codes "
                             f"(CODE_GENERATOR.CLS_LAYER kernel size {k}): cls_conv must be (N, 256, {k}, {k})")
        if self.owd:
            # `logits_pred = ones_like(logits_pred)[:, :, [0]]` after the sigmoid: one class whose probability is exactly 1 -- a zero
            # code with bias 40 (sigmoid(40) rounds to 1.0f) through the same class-conditional conv; the towers / box heads are unchanged.
            # The decode then runs with thresh_with_ctr = 1 (config_from_cfg): 1.0f * quality == quality exactly, so the candidates
            # are the locations whose quality alone clears the threshold, as in the reference (fcos_outputs.py:937)
            if getattr(self, "_owd_codes", None) is None:
                self._owd_codes = (torch.zeros(1, 256 * k * k, device=self.device), torch.full((1,), 40.0, device=self.device))
            w1, b1 = self._owd_codes
            self._ncls = 1
            check(self.L.sylph_fcos_head(self._ctx, _ptr(w1), _ptr(b1), 1), "fcos_head (OWD)")
            return
        # The codes of an episode are the same tensors for every query batch: their packed fp32 form is kept (no cast / reshape /
        # scale kernels in the steady-state step) until a different tensor, or a modified one, arrives.
        # Writes the library does through raw pointers (normalize_codes in place, ...) do not bump tensor._version: the engine
        # counts them (_lib_writes) and the count is part of the key, as are the CondConvBlock scales.
        key = (id(cls_conv), cls_conv._version, id(cls_bias), None if cls_bias is None else cls_bias._version, bool(raw),
               tuple(self.cond_scales), self._cond_scales_loaded, self._lib_writes)
        cached = getattr(self, "_codes_key", None) == key
        if not cached:
            self._codes = self._fold_codes(cls_conv, cls_bias, raw)
            self._codes_src = (cls_conv, cls_bias)  # keeps the ids alive
            self._codes_key = key
        w, b = self._codes
        self._ncls = w.size(0)
        check(self.L.sylph_fcos_head(self._ctx, _ptr(w), _ptr(b), self._ncls), "fcos_head")

    def head_episodes(self, codes, image_episode):
        """The head for a batch whose images belong to different episodes (sylph_fcos_head_episodes): `codes` is a list of
        (cls_conv (N_e, 256 k, 1, 1), cls_bias (N_e) or None), image i of the current batch is run with codes[image_episode[i]] and gets
        what `head(*codes[image_episode[i]])` gives it on the same batch.  `decode` then numbers classes within the image's own episode."""
        self._stream()
        if self.code_ksize != 1:
            raise NotImplementedError(f"head_episodes runs 1x1 class codes only: CODE_GENERATOR.CLS_LAYER kernel size {self.code_ksize} is not "
                                      "supported here (call head once per episode)")
        codes = [(w, b) for w, b in codes]
        image_episode = [int(e) for e in image_episode]
        if len(codes) == 0:
            raise ValueError("head_episodes needs at least one episode")
        if len(image_episode) != self._batch[0]:
            raise ValueError(f"image_episode has {len(image_episode)} entries for a batch of {self._batch[0]} images")
        if any(e < 0 or e >= len(codes) for e in image_episode):
            raise ValueError(f"image_episode entries must be in [0, {len(codes)})")
        for w, _ in codes:
            assert w.dim() == 4, f"Weight has dimension: {w.dim()}"
            assert w.size(2) == 1 and w.size(3) == 1
        if self.owd:  # the codes are not read (one all-ones class, see head): the uniform call
            return self.head(*codes[0])
        if len({b is None for _, b in codes}) != 1:
            raise ValueError("cls_bias must be given for every episode or for none")
        # the packed (sum N, 256) table is kept like head's single code set: no cast / concat kernels in a steady serving loop
        key = (tuple((id(w), w._version, id(b), None if b is None else b._version) for w, b in codes),
               tuple(self.cond_scales), self._cond_scales_loaded, self._lib_writes)
        if getattr(self, "_ep_codes_key", None) != key:
            folded = [self._fold_codes(w, b) for w, b in codes]
            W = torch.cat([w for w, _ in folded]).contiguous()
            Bv = torch.cat([b for _, b in folded]).contiguous() if folded[0][1] is not None else None
            self._ep_codes = (W, Bv, [int(w.size(0)) for w, _ in folded])
            self._ep_codes_src = codes  # keeps the ids alive
            self._ep_codes_key = key
        W, Bv, n = self._ep_codes
        self._ncls = max(n)
        check(self.L.sylph_fcos_head_episodes(self._ctx, len(n), _ptr(W), _ptr(Bv), _iarr(n), _iarr(image_episode)), "fcos_head_episodes")

    def head_code_sets(self, codes):
        """The head for a batch whose every image is scored against several code sets (sylph_fcos_head_codesets): `codes` is a list of
        (cls_conv (N_g, 256 k, 1, 1), cls_bias (N_g) or None).  The towers and box heads run once; `decode_code_sets` then returns for
        (set g, image i) what `head(*codes[g])` + `decode()` give image i on the same batch, classes numbered within set g."""
        self._stream()
        codes = [(w, b) for w, b in codes]
        check_code_sets(codes, self.code_ksize)
        if self.owd:  # the codes are not read (one all-ones class per set, see head)
            if getattr(self, "_owd_codes", None) is None:
                self._owd_codes = (torch.zeros(1, 256, device=self.device), torch.full((1,), 40.0, device=self.device))
            w1, b1 = self._owd_codes
            key, folded = ("owd", len(codes)), [(w1, b1)] * len(codes)
        else:
            for w, _ in codes:
                if w.size(1) != 256 and not self.is_roi_encoder:
                    raise ValueError(f"weight has wrong shape, {tuple(w.shape)}: feature.size(1) != weight.size(1) (256 channels expected)")
            key = (tuple((id(w), w._version, id(b), None if b is None else b._version) for w, b in codes),
                   tuple(self.cond_scales), self._cond_scales_loaded, self._lib_writes)
            folded = None
        # the packed (sum N, 256) table is kept like head's single code set: no cast / concat kernels in a steady serving loop
        if getattr(self, "_cs_codes_key", None) != key:
            if folded is None:
                folded = [self._fold_codes(w, b) for w, b in codes]
            W = torch.cat([w.reshape(w.size(0), -1) for w, _ in folded]).contiguous()
            Bv = torch.cat([b for _, b in folded]).contiguous() if folded[0][1] is not None else None
            self._cs_codes = (W, Bv, [int(w.size(0)) for w, _ in folded])
            self._cs_codes_src = codes  # keeps the ids alive
            self._cs_codes_key = key
        W, Bv, n = self._cs_codes
        self._ncls = sum(n)
        self._cs_n = list(n)
        check(self.L.sylph_fcos_head_codesets(self._ctx, len(n), _ptr(W), _ptr(Bv), _iarr(n)), "fcos_head_codesets")

    def decode_code_sets(self, out_sizes: Optional[List[Tuple[int, int]]] = None, max_out: Optional[int] = None):
        """After `head_code_sets`: -> [g][i] dicts with the fields of `decode` (sylph_decode_nms_codesets).  Raises on a status bit as
        `decode` does.  One device->host copy of the G * B counts."""
        self._stream()
        B = self._batch[0]
        G = len(getattr(self, "_cs_n", None) or [0])
        S = G * B
        if max_out is None:
            max_out = self.default_max_out()
        dev = self.device
        boxes = torch.empty(S, max_out, 4, device=dev)
        scores = torch.empty(S, max_out, device=dev)
        ints = torch.empty(3, S, max_out, device=dev, dtype=torch.int32)
        locs = torch.empty(S, max_out, 2, device=dev)
        counts = torch.empty(S + 1, device=dev, dtype=torch.int32)  # [S] = status word
        oh = _iarr([s[0] for s in out_sizes]) if out_sizes is not None else None
        ow = _iarr([s[1] for s in out_sizes]) if out_sizes is not None else None
        check(self.L.sylph_decode_nms_codesets(self._ctx, G, oh, ow, max_out, _ptr(boxes), _ptr(scores), _ptr(ints[0]), _ptr(ints[1]),
                                               _ptr(locs), _ptr(ints[2]), _ptr(counts), c_void_p(counts.data_ptr() + 4 * S)),
              "decode_nms_codesets")
        host_counts = self._counts_acquire(S + 1)  # pinned staging for the counts, as in decode_launch
        host_counts.copy_(counts, non_blocking=True)
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(dev))
        flat = self.decode_fetch((S, boxes, scores, ints, None, locs, None, host_counts, done, torch.cuda.current_stream(dev)))
        return [flat[g * B:(g + 1) * B] for g in range(G)]

    def head_pretrained(self) -> int:
        """forward_base_train (fcos.py:543-578): towers + the checkpoint's own cls_logits conv (1x1 or 3x3) -> number of classes."""
        self._stream()
        n = c_int(0)
        check(self.L.sylph_fcos_head_pretrained(self._ctx, ctypes.byref(n)), "fcos_head_pretrained")
        self._ncls = n.value
        return n.value

    def export_head(self):
        self._stream()
        B, H, W, _ = self._batch
        lo, rg, ct, io = [], [], [], []
        for l, (h, w) in enumerate(self.level_shapes(H, W)):
            a = torch.empty(B, self._ncls, h, w, device=self.device)
            r = torch.empty(B, 4, h, w, device=self.device)
            c = torch.empty(B, 1, h, w, device=self.device)
            q = torch.empty(B, 1, h, w, device=self.device)
            check(self.L.sylph_export_head(self._ctx, l, _ptr(a), _ptr(r), _ptr(c), _ptr(q)), "export_head")
            lo.append(a); rg.append(r); ct.append(c); io.append(q)
        return lo, rg, ct, io

    def import_head(self, logits: List[torch.Tensor], reg: List[torch.Tensor], ctr: List[torch.Tensor],
                    iou: Optional[List[torch.Tensor]] = None):
        """Test boundary: per-level fp32 NCHW head outputs -> the context (then `decode`)."""
        self._stream()
        N = int(logits[0].shape[1])
        keep = []
        for l in range(self.nlevels):
            ts = [t[l].to(self.device, torch.float32).contiguous() if t is not None else None for t in (logits, reg, ctr, iou)]
            keep.append(ts)
            check(self.L.sylph_import_head(self._ctx, N, l, _ptr(ts[0]), _ptr(ts[1]), _ptr(ts[2]), _ptr(ts[3])), "import_head")
        self._keep_head = keep
        self._ncls = N
        self._record = None

    def roi_align(self, boxes: torch.Tensor) -> torch.Tensor:
        """Test boundary: ROIPooler(7x7, ROIAlignV2) of one box per image of the current batch -> (S,256,7,7)."""
        self._stream()
        B = self._batch[0]
        bx = boxes.to(self.device, torch.float32).reshape(-1, 4).contiguous()
        assert bx.shape[0] == B
        out = torch.empty(B, 256, 7, 7, device=self.device)
        check(self.L.sylph_roi_align(self._ctx, _ptr(bx), _ptr(out)), "roi_align")
        return out

    def _check_rois(self, boxes: torch.Tensor, roi_image) -> Tuple[torch.Tensor, List[int]]:
        """The ROI list of a call against the current batch -> (boxes (R, 4) on the device, roi_image as ints)."""
        if getattr(self, "_batch", None) is None:
            raise ValueError("no current batch")
        if boxes is None or roi_image is None:
            raise ValueError("boxes and roi_image must be given")
        B = self._batch[0]
        ri = [int(i) for i in (roi_image.tolist() if torch.is_tensor(roi_image) else roi_image)]
        R = len(ri)
        if R < 1:
            raise ValueError("the ROI list is empty (R < 1)")
        if boxes.numel() != 4 * R:
            raise ValueError(f"boxes has {boxes.numel()} values for {R} ROIs: (R, 4) expected")
        for r, i in enumerate(ri):
            if i < 0 or i >= B:
                raise ValueError(f"roi_image[{r}] = {i} is outside the batch of {B} images")
        return boxes.to(self.device, torch.float32).reshape(R, 4).contiguous(), ri

    def roi_align_rois(self, boxes: torch.Tensor, roi_image) -> torch.Tensor:
        """Test boundary: the ROIPooler call over a ROI list, box r on image roi_image[r] of the current batch -> (R,256,7,7)."""
        self._stream()
        bx, ri = self._check_rois(boxes, roi_image)
        out = torch.empty(len(ri), 256, 7, 7, device=self.device)
        check(self.L.sylph_roi_align_rois(self._ctx, len(ri), _ptr(bx), _iarr(ri), _ptr(out)), "roi_align_rois")
        return out

    def decode(self, out_sizes: Optional[List[Tuple[int, int]]] = None, max_out: Optional[int] = None):
        """-> per image dict of device tensors (pred_boxes, scores, pred_classes, fpn_levels, locations,
        cand_index).  One device->host copy of the per-image counts (the only sync of a query step)."""
        return self.decode_fetch(self.decode_launch(out_sizes, max_out))

    def default_max_out(self) -> int:
        """Detection rows per image that decode reserves when the caller passes no max_out."""
        K = int(self.sc.post_nms_topk)
        return 2 * K if K > 0 else int(self.sc.pre_nms_topk) * self.nlevels

    def decode_launch(self, out_sizes: Optional[List[Tuple[int, int]]] = None, max_out: Optional[int] = None):
        """Enqueue decode + NMS on the current stream and return a handle WITHOUT synchronising: the caller can
        launch the next batch (another Engine on another stream) before `decode_fetch` reads the counts back.

        The in-flight contract (tests/test_steps_in_flight_gpu.py):
          * any number of handles may be outstanding, and they may be fetched in any order, each once; a handle carries its own counts
            and its own status word, so `decode_fetch` raises for the step that overflowed and for no other;
          * every entry runs on torch's current stream.  While handles are outstanding the engine stays on one stream, or the caller
            orders the streams itself (`new.wait_stream(old)`) before it switches; `decode_fetch` may run on any stream (it makes
            the current stream wait for the handle's);
          * the caller keeps the tensors it passed in (images, class codes) alive until the step that reads them has been fetched:
            the library reads device images through the caller's pointers when the step runs, not when it is enqueued.  Writing
            into them in place is fine when the write is ordered on the engine's stream (a `copy_` there is seen by the steps
            enqueued after it and by none before it)."""
        self._stream()
        B = self._batch[0]
        if max_out is None:
            max_out = self.default_max_out()
        dev = self.device
        boxes = torch.empty(B, max_out, 4, device=dev)
        scores = torch.empty(B, max_out, device=dev)
        ints = torch.empty(3, B, max_out, device=dev, dtype=torch.int32)  # classes | levels | candidate ordinals: ONE widening later
        classes, levels, cand = ints[0], ints[1], ints[2]
        locs = torch.empty(B, max_out, 2, device=dev)
        counts = torch.empty(B + 1, device=dev, dtype=torch.int32)  # [B] = status word
        oh = _iarr([s[0] for s in out_sizes]) if out_sizes is not None else None
        ow = _iarr([s[1] for s in out_sizes]) if out_sizes is not None else None
        check(self.L.sylph_decode_nms(self._ctx, oh, ow, max_out, _ptr(boxes), _ptr(scores), _ptr(classes),
                                      _ptr(levels), _ptr(locs), _ptr(cand), _ptr(counts),
                                      c_void_p(counts.data_ptr() + 4 * B)), "decode_nms")
        host_counts = self._counts_acquire(B + 1)  # pinned staging for the counts: this handle's until decode_fetch has read it
        host_counts.copy_(counts, non_blocking=True)
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(dev))
        return (B, boxes, scores, ints, None, locs, None, host_counts, done, torch.cuda.current_stream(dev))

    def _counts_acquire(self, n: int) -> torch.Tensor:
        """A pinned (n,) int32 staging buffer for one decode's counts and status word.  It belongs to the handle that carries it from
        the launch until decode_fetch has read it, however many decodes are launched in between; fetched buffers are reused, and a new
        one is allocated only when none of that length is free (a fresh pinned allocation costs milliseconds of host time, which is the
        whole step at batch 1): a serving loop with k steps in flight allocates k buffers and then none."""
        free = self._counts_free.setdefault(n, [])
        buf = free.pop() if free else torch.empty(n, dtype=torch.int32, pin_memory=True)
        self._counts_out.add(id(buf))
        return buf

    def _counts_release(self, buf: torch.Tensor):
        self._counts_out.discard(id(buf))
        self._counts_free.setdefault(buf.numel(), []).append(buf)

    def decode_fetch(self, handle):
        B, boxes, scores, ints, _, locs, _, host_counts, done, stream = handle
        if id(host_counts) not in self._counts_out:
            raise RuntimeError("sylph decode_fetch: this handle has been fetched already (or belongs to another Engine)")
        done.synchronize()
        cnt = host_counts.tolist()
        self._counts_release(host_counts)  # read: the buffer is free for the next launch, whatever the status word says
        status = cnt[B]
        if status & 1:
            raise RuntimeError("sylph decode: per-level candidate capacity exceeded (raise cand_cap)")
        if status & 2:
            raise RuntimeError("sylph decode: more tied detections than max_out")
        with torch.cuda.stream(stream):
            wide = ints.long()  # one launch (the reference's index tensors are int64), then views only
            classes, levels, cand = wide[0], wide[1], wide[2]
        cur = torch.cuda.current_stream(self.device)
        if cur != stream:
            cur.wait_stream(stream)
        # B x 6 views: one unbind per tensor + one narrow per view (boxes[i, :n] is two indexing calls per view: 43 -> 19 us per image
        # of host time on the critical path of a synchronous step)
        nar = torch.Tensor.narrow
        cols = [[nar(r, 0, 0, n) for r, n in zip(t.unbind(0), cnt)] for t in (boxes, scores, classes, levels, locs, cand)]
        keys = ("pred_boxes", "scores", "pred_classes", "fpn_levels", "locations", "cand_index")
        return [dict(zip(keys, vals)) for vals in zip(*cols)]

    # ---- views: per-view rows of several steps, merged per source ------------------------------------------
    def new_view_rows(self, n_views: int, max_in: Optional[int] = None) -> Dict:
        """Row buffers [n_views][max_in] for the detections of n_views views: every step's `decode_rows` fills the slice of its views."""
        if max_in is None:
            max_in = self.default_max_out()
        dev = self.device
        ints = torch.empty(3, n_views, max_in, device=dev, dtype=torch.int32)  # classes | levels | candidate ordinals
        meta = torch.zeros(2 * n_views, device=dev, dtype=torch.int32)         # counts [n_views] | status word of every decode
        return {"n_views": n_views, "max_in": int(max_in), "boxes": torch.empty(n_views, max_in, 4, device=dev),
                "scores": torch.empty(n_views, max_in, device=dev), "classes": ints[0], "levels": ints[1], "cand": ints[2],
                "locations": torch.empty(n_views, max_in, 2, device=dev), "meta": meta, "counts": meta[:n_views], "steps": 0}

    def decode_rows(self, rows: Dict, row0: int, out_sizes: Optional[List[Tuple[int, int]]] = None):
        """decode + NMS of the current batch into rows [row0, row0 + B) of `rows` (decode writes [B][max_out] rows, so the steps of a
        view list land in consecutive slices).  Nothing is read back: `merge_views` fetches every step's status with the counts."""
        self._stream()
        B, n, m = self._batch[0], rows["n_views"], rows["max_in"]
        if row0 < 0 or row0 + B > n:
            raise ValueError(f"rows [{row0}, {row0 + B}) are outside the {n} view rows")
        oh = _iarr([s[0] for s in out_sizes]) if out_sizes is not None else None
        ow = _iarr([s[1] for s in out_sizes]) if out_sizes is not None else None
        sl = lambda t: c_void_p(t[row0:].data_ptr())
        check(self.L.sylph_decode_nms(self._ctx, oh, ow, m, sl(rows["boxes"]), sl(rows["scores"]), sl(rows["classes"]), sl(rows["levels"]),
                                      sl(rows["locations"]), sl(rows["cand"]), sl(rows["counts"]),
                                      c_void_p(rows["meta"].data_ptr() + 4 * (n + rows["steps"]))), "decode_nms")
        rows["steps"] += 1

    def merge_views(self, view_table: List[Dict], rows: Dict, max_out: Optional[int] = None, n_src: Optional[int] = None):
        """One class-wise NMS over the views of every source (sylph_merge_views).  view_table[v] = {"source", "crop", "flip"} describes
        view v, whose detections are rows["boxes" | "scores" | "classes"][v, :rows["counts"][v]] ([n_views][max_in]; classes int32), in
        crop pixels.  -> per source a dict of pred_boxes (source pixels), scores, pred_classes, view_index, view_row (the input row of
        each output).  One device->host copy: the merged counts with the status words of the merge and of every decode_rows step."""
        return self._merge_views(view_table, rows, max_out, n_src, None, large=False)

    def merge_views_large(self, view_table: List[Dict], rows: Dict, max_out: Optional[int] = None, n_src: Optional[int] = None,
                          topk: Optional[int] = None):
        """`merge_views` for sources of any size (sylph_merge_views_large: up to MERGE_LARGE_POOL_CAP rows per source, the pool in a
        workspace this engine owns and grows on demand): the same result, the same read-back, the same errors.  topk is rule 5's K for
        this call: a count, 0 = every kept box, None = POST_NMS_TOPK_TEST."""
        return self._merge_views(view_table, rows, max_out, n_src, -1 if topk is None else int(topk), large=True)

    def stitch_views(self, view_table: List[Dict], rows: Dict, source_sizes: Sequence[Tuple[int, int]], stitch_thr: float = 0.5,
                     border_px: float = 2.0, max_out: Optional[int] = None, n_src: Optional[int] = None, topk: Optional[int] = None):
        """`merge_views_large` that also stitches what tile borders cut (sylph_stitch_views; the rules stand in include/sylph_hip.h): a row
        within border_px of a crop border that lies inside its source is cut; a cut row joins the first kept box of its class that shares
        more than stitch_thr of the smaller of the two, whose box grows to their hull.  source_sizes[s] = (height, width) of source s.
        -> merge_views_large's dicts plus "stitched": the rows each output stands for, itself included.  The workspace is the
        engine's own, as for the large merge."""
        return self._merge_views(view_table, rows, max_out, n_src, -1 if topk is None else int(topk), large=True,
                                 stitch=(list(source_sizes), float(stitch_thr), float(border_px)))

    def _merge_views(self, view_table, rows, max_out, n_src, topk, large: bool, stitch=None):
        self._stream()
        nv = len(view_table)
        boxes, scores, classes, counts = rows["boxes"], rows["scores"], rows["classes"], rows["counts"]
        max_in = int(scores.shape[1])
        if scores.shape[0] != nv or counts.numel() != nv:
            raise ValueError(f"the view table has {nv} views, the row buffers {scores.shape[0]}")
        assert boxes.dtype == torch.float32 and scores.dtype == torch.float32 and classes.dtype == torch.int32 and counts.dtype == torch.int32
        assert boxes.is_contiguous() and scores.is_contiguous() and classes.is_contiguous() and counts.is_contiguous()
        src = [int(v["source"]) for v in view_table]
        if n_src is None:
            n_src = max(src) + 1
        if max_out is None:
            max_out = self.default_max_out()
        dev = self.device
        farr = lambda v: (ctypes.c_float * len(v))(*[float(x) for x in v])
        ob = torch.empty(n_src, max_out, 4, device=dev)
        osc = torch.empty(n_src, max_out, device=dev)
        oi = torch.empty(3, n_src, max_out, device=dev, dtype=torch.int32)  # classes | view | row
        steps = int(rows.get("steps", 0))
        tail = torch.empty(n_src + 1 + steps, device=dev, dtype=torch.int32)  # merged counts | merge status | decode status words
        tables = (n_src, nv, _iarr(src), farr([v["crop"][0] for v in view_table]), farr([v["crop"][1] for v in view_table]),
                  farr([v["crop"][2] for v in view_table]), _iarr([1 if v.get("flip", False) else 0 for v in view_table]), max_in,
                  _ptr(boxes), _ptr(scores), _ptr(classes), _ptr(counts))
        outs = (max_out, _ptr(ob), _ptr(osc), _ptr(oi[0]), _ptr(oi[1]), _ptr(oi[2]), _ptr(tail), c_void_p(tail.data_ptr() + 4 * n_src))
        if stitch is not None:
            sizes, sthr, border = stitch
            if len(sizes) != n_src:
                raise ValueError(f"stitch_views: {len(sizes)} source sizes for {n_src} sources")
            ost = torch.empty(n_src, max_out, device=dev, dtype=torch.int32)
            need = int(self.L.sylph_stitch_views_bytes(n_src, nv, max_in))
            ws = self._merge_ws
            if need > 0 and (ws is None or ws.numel() < need):  # (a refused size: the entry names the reason)
                ws = self._merge_ws = torch.empty(need, device=dev, dtype=torch.uint8)
            t = tables
            check(self.L.sylph_stitch_views(self._ctx, *t[:6], farr([v["crop"][3] for v in view_table]), t[6], farr([hw[1] for hw in sizes]),
                                            farr([hw[0] for hw in sizes]), *t[7:], sthr, border, topk, *outs[:6], _ptr(ost), *outs[6:],
                                            _ptr(ws) if ws is not None else None, ws.numel() if ws is not None else 0), "stitch_views")
        elif large:
            need = int(self.L.sylph_merge_views_large_bytes(n_src, nv, max_in))
            ws = self._merge_ws
            if need > 0 and (ws is None or ws.numel() < need):  # (a refused size: the entry names the reason)
                ws = self._merge_ws = torch.empty(need, device=dev, dtype=torch.uint8)
            check(self.L.sylph_merge_views_large(self._ctx, *tables, topk, *outs, _ptr(ws) if ws is not None else None,
                                                 ws.numel() if ws is not None else 0), "merge_views_large")
        else:
            check(self.L.sylph_merge_views(self._ctx, *tables, *outs), "merge_views")
        if steps:
            tail[n_src + 1:].copy_(rows["meta"][nv:nv + steps])
        cnt = tail.tolist()  # the only sync
        for st in cnt[n_src + 1:]:
            if st & 1:
                raise RuntimeError("sylph decode: per-level candidate capacity exceeded (raise cand_cap)")
            if st & 2:
                raise RuntimeError("sylph decode: more tied detections than max_out")
        if cnt[n_src] & 2:
            raise RuntimeError("sylph merge_views: more detections of a source than max_out")
        wide = oi.long()
        out = []
        for s_ in range(n_src):
            k = cnt[s_]
            out.append({"pred_boxes": ob[s_, :k], "scores": osc[s_, :k], "pred_classes": wide[0, s_, :k], "view_index": wide[1, s_, :k],
                        "view_row": wide[2, s_, :k]})
            if stitch is not None:
                out[-1]["stitched"] = ost[s_, :k].long()
        return out

    # ---- support path -------------------------------------------------------------------------------
    def _image_boxes(self, boxes: torch.Tensor) -> torch.Tensor:
        """One box per image of the current batch -> (B, 4) fp32 on the device; the message is the reference's."""
        bx = boxes.to(self.device, torch.float32).reshape(-1, 4).contiguous()
        B = self._batch[0]
        assert bx.shape[0] == B, f"pooled_features.shape[0] {bx.shape[0]} Vs batch_size * num_shots {B}"
        return bx

    def _run_codegen(self, what: str, bx: torch.Tensor, n_codes: Optional[int], *args) -> torch.Tensor:
        """The common end of the three codegen* methods, their arguments checked: sylph_<what>(ctx, *args, out) on the device boxes bx, which
        stay alive while the library reads them -> n_codes rows of code_len floats (None: one bare row)."""
        self._stream()
        out = torch.empty(*(() if n_codes is None else (n_codes,)), self.code_len, device=self.device)
        self._keep_boxes = bx
        check(getattr(self.L, "sylph_" + what)(self._ctx, *args, _ptr(out)), what)
        self._sup_rows = bx.shape[0]
        return out

    def codegen(self, boxes: torch.Tensor) -> torch.Tensor:
        bx = self._image_boxes(boxes)
        B = bx.shape[0]
        if B > 64:
            raise ValueError(f"{B} support images of one class in one call: the code generator's shot reduction handles at most 64 "
                             "(split the class into chunks and reduce them, as the base-class path does)")
        return self._run_codegen("codegen", bx, None, _ptr(bx))

    def codegen_classes(self, boxes: torch.Tensor, shots: int) -> torch.Tensor:
        """Several classes in ONE batch: the current batch holds n_classes * shots support images (class k = images
        [k * shots, (k + 1) * shots)), boxes (n_classes * shots, 4) -> (n_classes, 256 k^2 + 1) un-normalised codes (k = code_ksize)."""
        bx = self._image_boxes(boxes)
        B = bx.shape[0]
        assert B % shots == 0, f"pooled_features.shape[0] {B} Vs batch_size * num_shots {B}"
        if shots > 64:
            raise ValueError(f"{shots} shots per class in one call: the code generator's shot reduction handles at most 64 (split the "
                             "class into chunks and reduce them, as the base-class path does)")
        return self._run_codegen("codegen_classes", bx, B // shots, _ptr(bx), int(shots))

    def codegen_rois(self, boxes: torch.Tensor, roi_image, seg_len) -> torch.Tensor:
        """Class codes from a ROI list over the current batch (sylph_codegen_rois): ROI r is boxes[r] on image roi_image[r], any
        number per image in any order; the ROIs are cut into consecutive segments of seg_len[j] >= 1 shots and row j of the
        (n_seg, 256 k^2 + 1) result is the un-normalised code of segment j, as `codegen` gives it for a batch holding the segment's images
        once per ROI.  No cap on a segment's length."""
        bx, ri = self._check_rois(boxes, roi_image)
        if seg_len is None:
            raise ValueError("seg_len must be given")
        sl = [int(n) for n in (seg_len.tolist() if torch.is_tensor(seg_len) else seg_len)]
        if len(sl) < 1:
            raise ValueError("the ROI list has no segment (n_seg < 1)")
        for j, n in enumerate(sl):
            if n < 1:
                raise ValueError(f"seg_len[{j}] = {n}: a segment needs at least one ROI")
        if sum(sl) != len(ri):
            raise ValueError(f"the segment lengths sum to {sum(sl)}, not to R = {len(ri)}")
        return self._run_codegen("codegen_rois", bx, len(sl), len(ri), _ptr(bx), _iarr(ri), len(sl), _iarr(sl))

    # ---- shot bank (sylph_amd.shots.ShotBank) ----
    @property
    def shot_row_floats(self) -> int:
        """Floats of one shot-bank row under this engine's config (sylph_shot_row_floats)."""
        n = c_int(0)
        check(self.L.sylph_shot_row_floats(self._ctx, ctypes.byref(n)), "shot_row_floats")
        return n.value

    def shot_key(self) -> Dict[str, Any]:
        """What a bank's rows depend on besides the weights: generator type, code kernel size, dtype, row width."""
        return {"generator": "ROIEncoder" if self.is_roi_encoder else "CodeGenerator", "code_ksize": self.code_ksize,
                "dtype": "f32" if self.dtype == "fp32" else self.dtype, "row_floats": self.shot_row_floats}

    def codegen_shots(self, boxes: torch.Tensor, roi_image) -> torch.Tensor:
        """The per-shot rows of the ROI list over the current batch (sylph_codegen_shots) -> (R, shot_row_floats) fp32: everything
        codegen_rois computes from one ROI alone.  combine_shots turns any list of such rows into class codes."""
        bx, ri = self._check_rois(boxes, roi_image)
        self._stream()
        out = torch.empty(len(ri), self.shot_row_floats, device=self.device)
        self._keep_boxes = bx
        check(self.L.sylph_codegen_shots(self._ctx, len(ri), _ptr(bx), _iarr(ri), _ptr(out)), "codegen_shots")
        self._sup_rows = len(ri)
        return out

    def combine_shots(self, rows: torch.Tensor, idx, seg_len) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """Class codes of segments drawn from bank rows (sylph_shot_combine): idx (M) row numbers, repeats allowed, cut into consecutive
        segments of seg_len[j] >= 1 -> ((n_seg, 256 k^2 + 1) un-normalised codes, (n_seg,) cls_weight_norm or None without a
        SCALE_LAYER): bit for bit what codegen_rois gives for segments holding those shots in that order.  Needs no current batch."""
        if rows is None or idx is None or seg_len is None:
            raise ValueError("rows, idx and seg_len must be given")
        if not (torch.is_tensor(rows) and rows.is_cuda and rows.dtype == torch.float32 and rows.dim() == 2 and rows.is_contiguous()):
            raise ValueError("rows must be a contiguous 2-d fp32 tensor on the device")
        if rows.shape[1] != self.shot_row_floats:
            raise ValueError(f"bank rows of {rows.shape[1]} floats on an engine whose shot rows are {self.shot_row_floats} floats wide "
                             f"({'ROIEncoder' if self.is_roi_encoder else 'CodeGenerator'}, code kernel size {self.code_ksize})")
        ix = [int(i) for i in (idx.tolist() if torch.is_tensor(idx) or hasattr(idx, "tolist") else idx)]
        sl = [int(n) for n in (seg_len.tolist() if torch.is_tensor(seg_len) or hasattr(seg_len, "tolist") else seg_len)]
        if len(sl) < 1:
            raise ValueError("the draw has no segment (n_seg < 1)")
        for i, v in enumerate(ix):
            if v < 0 or v >= rows.shape[0]:
                raise ValueError(f"idx[{i}] = {v} is outside the bank of {rows.shape[0]} rows")
        for j, n in enumerate(sl):
            if n < 1:
                raise ValueError(f"seg_len[{j}] = {n}: a segment needs at least one shot")
        if sum(sl) != len(ix):
            raise ValueError(f"the segment lengths sum to {sum(sl)}, not to M = {len(ix)}")
        self._stream()
        codes = torch.empty(len(sl), self.code_len, device=self.device)
        wn = torch.empty(len(sl), device=self.device) if (not self.is_roi_encoder and int(self.sc.cg_has_scale)) else None
        check(self.L.sylph_shot_combine(self._ctx, _ptr(rows), rows.shape[0], len(ix), _iarr(ix), len(sl), _iarr(sl), _ptr(codes), _ptr(wn)),
              "shot_combine")
        return codes, wn

    # ---- meta-training of the code generator (sylph_amd/metatrain.py) ------------------------------------------------------------------

    def roi_rows(self, boxes: torch.Tensor, roi_image) -> torch.Tensor:
        """The ROI bank rows of a ROI list over the current batch (sylph_roi_rows) -> (R, 49, 256) bf16, position-major: the values of
        roi_align_rois, written in one launch.  They depend on the backbone alone."""
        bx, ri = self._check_rois(boxes, roi_image)
        self._stream()
        out = torch.empty(len(ri), 49, 256, device=self.device, dtype=torch.bfloat16)
        self._keep_boxes = bx
        check(self.L.sylph_roi_rows(self._ctx, len(ri), _ptr(bx), _iarr(ri), _ptr(out)), "roi_rows")
        return out

    def codegen_params(self) -> List[Tuple[str, int, int]]:
        """(state-dict key, offset, element count) of the generator's trainable tensors in the flat fp32 vector (sylph_codegen_param_layout)."""
        n, total = c_int(0), c_int64(0)
        check(self.L.sylph_codegen_param_layout(self._ctx, 0, None, None, None, ctypes.byref(n), ctypes.byref(total)), "codegen_param_layout")
        keys = ctypes.create_string_buffer(128 * n.value)
        off, cnt = (c_int64 * n.value)(), (c_int64 * n.value)()
        check(self.L.sylph_codegen_param_layout(self._ctx, n.value, keys, off, cnt, ctypes.byref(n), ctypes.byref(total)), "codegen_param_layout")
        return [(keys.raw[128 * i:128 * (i + 1)].split(b"\0", 1)[0].decode(), int(off[i]), int(cnt[i])) for i in range(n.value)]

    @staticmethod
    def codegen_param_shape(key: str, numel: int) -> Tuple[int, ...]:
        """torch shape of a layout entry"""
        if key.endswith(".weight") and numel % 2304 == 0:
            return (numel // 2304, 256, 3, 3)
        return (numel,)

    def codegen_flat_size(self) -> int:
        lay = self.codegen_params()
        return lay[-1][1] + lay[-1][2]

    def code_generator(self) -> torch.Tensor:
        """The checkpoint's generator as the flat fp32 vector of codegen_params() (CPU)."""
        flat = torch.empty(self.codegen_flat_size(), dtype=torch.float32)
        check(self.L.sylph_get_code_generator(self._ctx, ctypes.cast(flat.data_ptr(), ctypes.POINTER(ctypes.c_float))), "get_code_generator")
        return flat

    def codegen_stamp(self) -> int:
        """0 while the support path runs the checkpoint's generator, else the stamp of the set_code_generator that installed the current one"""
        st = ctypes.c_uint64(0)
        check(self.L.sylph_codegen_stamp(self._ctx, ctypes.byref(st)), "codegen_stamp")
        return st.value

    def set_code_generator(self, flat):
        """Install a generator (the flat vector of codegen_params(), or a dict of its state-dict entries; None: the checkpoint's).  From the
        next support pass on every codegen* / normalize_codes result is bit-identical to an engine loaded with a state dict carrying these
        tensors.  The current batch and query records stay as they are; shot banks built under another generator are refused."""
        self._stream()
        if flat is None:
            check(self.L.sylph_set_code_generator(self._ctx, None), "set_code_generator")
            return
        if isinstance(flat, dict):
            vec = self.code_generator()
            for k, o, n in self.codegen_params():
                if k in flat:
                    vec[o:o + n] = flat[k].detach().to("cpu", torch.float32).reshape(-1)
            flat = vec
        flat = torch.as_tensor(flat).detach().to("cpu", torch.float32).reshape(-1).contiguous()
        if flat.numel() != self.codegen_flat_size():
            raise ValueError(f"set_code_generator: the flat vector holds {self.codegen_flat_size()} floats under this config, got {flat.numel()}")
        check(self.L.sylph_set_code_generator(self._ctx, ctypes.cast(flat.data_ptr(), ctypes.POINTER(ctypes.c_float))), "set_code_generator")

    def codegen_train_shape(self, M: int, n_seg: int) -> Dict[str, int]:
        """units / passes of the weight gradient's reduction and the floats of the debug export for a step of M shots in n_seg classes"""
        u, p, d = c_int(0), c_int(0), c_int64(0)
        check(self.L.sylph_codegen_train_shape(self._ctx, int(M), int(n_seg), ctypes.byref(u), ctypes.byref(p), ctypes.byref(d)), "codegen_train_shape")
        return {"units": u.value, "passes": p.value, "debug_floats": d.value}

    def codegen_train_forward(self, params: torch.Tensor, rows: torch.Tensor, idx, seg_len) -> torch.Tensor:
        """Training-mode forward of the generator (sylph_codegen_train_forward): params the flat fp32 device vector, rows the (n_rows, 49,
        256) bf16 ROI bank, idx (M) bank rows cut into consecutive segments of seg_len shots -> (n_seg, 257) normalised code ++ processed
        bias.  The saved activations stay in a workspace of the engine until the backward.  Needs no current batch."""
        if not (torch.is_tensor(params) and params.is_cuda and params.dtype == torch.float32 and params.is_contiguous()):
            raise ValueError("codegen_train_forward: params must be a contiguous fp32 tensor on the device")
        if not (torch.is_tensor(rows) and rows.is_cuda and rows.dtype == torch.bfloat16 and rows.is_contiguous() and tuple(rows.shape[1:]) == (49, 256)):
            raise ValueError("codegen_train_forward: rows must be a contiguous (n_rows, 49, 256) bf16 tensor on the device")
        ix = [int(i) for i in (idx.tolist() if hasattr(idx, "tolist") else idx)]
        sl = [int(n) for n in (seg_len.tolist() if hasattr(seg_len, "tolist") else seg_len)]
        self._stream()
        need = c_int64(0)
        check(self.L.sylph_codegen_train_bytes(self._ctx, len(ix), len(sl), ctypes.byref(need)), "codegen_train_bytes")
        if params.numel() != self.codegen_flat_size():
            raise ValueError(f"codegen_train_forward: params holds {params.numel()} floats, the layout {self.codegen_flat_size()}")
        ws = self._grow_ws("_cgt_ws", need.value)
        codes = torch.empty(len(sl), 257, device=self.device)
        check(self.L.sylph_codegen_train_forward(self._ctx, _ptr(params), _ptr(rows), rows.shape[0], len(ix), _iarr(ix), len(sl), _iarr(sl),
                                                 _ptr(ws), _ptr(codes)), "codegen_train_forward")
        self._cgt_last = (params, rows, len(ix), len(sl))
        return codes

    def codegen_train_backward(self, grad_codes: torch.Tensor, debug: bool = False):
        """Backward of the preceding codegen_train_forward: grad_codes (n_seg, 257) = d loss / d codes -> the flat gradient (device, the
        layout of codegen_params()); with debug -> (grad, stages), stages a dict of every exported stage in fp32 (see include/sylph_hip.h)."""
        last = getattr(self, "_cgt_last", None)
        if last is None:
            raise ValueError("codegen_train_backward: no codegen_train_forward precedes it")
        params, rows, M, n_seg = last
        g = torch.as_tensor(grad_codes).to(self.device, torch.float32).contiguous()
        if tuple(g.shape) != (n_seg, 257):
            raise ValueError(f"codegen_train_backward: grad_codes must be ({n_seg}, 257), got {tuple(g.shape)}")
        self._stream()
        grad = torch.empty_like(params)
        dbg = torch.empty(self.codegen_train_shape(M, n_seg)["debug_floats"], device=self.device) if debug else None
        check(self.L.sylph_codegen_train_backward(self._ctx, _ptr(params), _ptr(rows), rows.shape[0], M, n_seg, _ptr(self._cgt_ws), _ptr(g),
                                                  _ptr(grad), _ptr(dbg)), "codegen_train_backward")
        self._keep_cgt = g
        if not debug:
            return grad
        L, R = int(self.sc.cg_tower_layers), M * 49
        st, o = {}, 0

        def take(name, *shape):
            nonlocal o
            n = 1
            for s in shape:
                n *= s
            st[name] = dbg[o:o + n].view(*shape)
            o += n
        for i in range(L):
            take(f"y{i}", R, 256)
            take(f"stats{i}", M, 32, 2)
            take(f"x{i + 1}", R, 256)
        take("xsum", M, 2304); take("c", M, 256); take("rb", M); take("code_raw", n_seg, 256); take("bias_raw", n_seg)
        take("d_code_raw", n_seg, 256); take("d_bias_raw", n_seg); take("d_c", M, 256); take("d_rb", M)
        if L:
            take("d_xsum", M, 2304)
            take(f"d_x{L}", R, 256)
            for i in range(L - 1, -1, -1):
                take(f"d_y{i}", R, 256)
                if i >= 1:
                    take(f"d_x{i}", R, 256)
        assert o == dbg.numel()
        return grad, st

    def roi_table_uploads(self) -> int:
        """How many codegen* calls of this engine uploaded their ROI tables (a repeated identical list uploads none)."""
        n = c_int64(0)
        check(self.L.sylph_roi_table_uploads(self._ctx, ctypes.byref(n)), "roi_table_uploads")
        return n.value

    def codegen_weight_norm(self, n_classes: int = 1) -> torch.Tensor:
        """cls_weight_norm of the last codegen / codegen_classes / codegen_rois call (CODE_GENERATOR.SCALE_LAYER), one value per
        class (per segment after codegen_rois)."""
        self._stream()
        out = torch.empty(n_classes, device=self.device)
        check(self.L.sylph_codegen_weight_norm(self._ctx, _ptr(out)), "codegen_weight_norm")
        return out

    def normalize_codes(self, codes: torch.Tensor, weight_norm: Optional[torch.Tensor] = None) -> torch.Tensor:
        self._stream()
        assert codes.is_cuda and codes.dtype == torch.float32 and codes.is_contiguous()
        if codes.shape[-1] != self.code_len:
            raise ValueError(f"normalize_codes: rows of {codes.shape[-1]} floats on an engine whose codes are {self.code_ksize}x{self.code_ksize} "
                             f"({self.code_len} floats per row; CODE_GENERATOR.CLS_LAYER kernel size {self.code_ksize})")
        wn = None
        if weight_norm is not None:
            wn = weight_norm.to(self.device, torch.float32).reshape(-1).contiguous()
            assert wn.numel() == codes.shape[0]
        check(self.L.sylph_normalize_codes(self._ctx, _ptr(codes), codes.shape[0], _ptr(wn)), "normalize_codes")
        self._lib_writes += 1  # `codes` changed in place without a torch version bump
        return codes

    def reduce_codes(self, rows: torch.Tensor, num_classes: int, divide_by_acc: bool = True) -> torch.Tensor:  # (1x1 codes only: the C entry refuses cg_code_ksize 3)
        """Device-side reduce_class_code on packed rows (sylph_amd.distributed row layout) -> (num_classes, ROW), row c = class c.
        divide_by_acc False: plain per-class accumulation (the per-rank step of the base-class path)."""
        self._stream()
        assert rows.is_cuda and rows.dtype == torch.float32 and rows.dim() == 2 and rows.is_contiguous()
        out = torch.empty(num_classes, rows.shape[1], device=self.device)
        check(self.L.sylph_reduce_codes(self._ctx, _ptr(rows), rows.shape[0], rows.shape[1], _ptr(out), num_classes,
                                        int(divide_by_acc)), "reduce_codes")
        return out

    # ---- COCO bbox evaluation (sylph_amd.coco_eval.DeviceCOCOEvaluator) ----------------------------------
    def coco_match(self, det_rows: torch.Tensor, det_off: torch.Tensor, gt: Dict[str, torch.Tensor], n_cat: int, iou_thr: torch.Tensor,
                   area_rng: torch.Tensor, max_det: int):
        """sylph_coco_match: det_rows (n, 8) fp32 ordered by (pair, score descending), det_off [pairs + 1] int32; gt: the device table
        {"box" (G, 4) f64 XYWH, "area" f64, "crowd" int32, "off" [pairs + 1] int32, "max_per_pair" int} ordered by (pair, file order)
        -> (matched, ignored) int64 [n] (bit a * T + t), npig int32 [n_cat, areas].  Nothing is read back."""
        self._stream()
        n, n_pairs = det_rows.shape[0], det_off.numel() - 1
        assert det_rows.is_cuda and det_rows.dtype == torch.float32 and det_rows.is_contiguous() and (n == 0 or det_rows.shape[1] == 8)
        assert det_off.dtype == torch.int32 and gt["off"].dtype == torch.int32 and gt["off"].numel() == n_pairs + 1
        assert iou_thr.dtype == torch.float64 and area_rng.dtype == torch.float64 and area_rng.is_contiguous()
        matched = torch.zeros(n, dtype=torch.int64, device=self.device)
        ignored = torch.zeros(n, dtype=torch.int64, device=self.device)
        npig = torch.empty(n_cat, area_rng.shape[0], dtype=torch.int32, device=self.device)
        max_gt = int(gt["max_per_pair"])
        scratch = None
        tile_gt = self.L.sylph_coco_match_tile_gt(int(max_det))  # COCO_MATCH_TILE_GT, fewer for maxDets[-1] > 131; -1: the entry refuses max_det
        if tile_gt < 0 or max_gt > tile_gt:
            scratch = torch.empty(gt["box"].shape[0] * 64, dtype=torch.uint8, device=self.device)
        check(self.L.sylph_coco_match(self._ctx, n, _ptr(det_rows), n_pairs, n_cat, _ptr(det_off), _ptr(gt["box"]), _ptr(gt["area"]),
                                      _ptr(gt["crowd"]), _ptr(gt["off"]), max_gt, iou_thr.numel(), _ptr(iou_thr), area_rng.shape[0],
                                      _ptr(area_rng), int(max_det), _ptr(scratch), _ptr(matched), _ptr(ignored), _ptr(npig)), "coco_match")
        return matched, ignored, npig

    def lvis_match(self, det_rows: torch.Tensor, pairs: Dict[str, torch.Tensor], gt: Dict[str, torch.Tensor], n_cat: int, iou_thr: torch.Tensor,
                   area_rng: torch.Tensor, max_det: int):
        """sylph_lvis_match: det_rows (n, 8) fp32 ordered by (pair, score descending, arrival); pairs: the compacted pair list
        {"n" int32 [1] the live count (stays on the device), "cat", "flags" int32 [P], "det_off", "gt_off" int32 [P + 1]}, P a host-known upper
        bound; gt: {"box" (G, 4) f64 XYWH, "area" f64, "ignore" int32, "max_per_pair" int} ordered by (pair, file order); max_det: the most
        detections a pair can hold (max_dets_per_image) -> (matched, ignored) int64 [n], npig int32 [n_cat, areas].  Nothing is read back."""
        self._stream()
        n, P = det_rows.shape[0], pairs["cat"].numel()
        assert det_rows.is_cuda and det_rows.dtype == torch.float32 and det_rows.is_contiguous() and (n == 0 or det_rows.shape[1] == 8)
        assert all(pairs[k].dtype == torch.int32 and pairs[k].is_cuda and pairs[k].is_contiguous() for k in ("n", "cat", "flags", "det_off", "gt_off"))
        assert P > 0 and pairs["flags"].numel() == P and pairs["det_off"].numel() == P + 1 and pairs["gt_off"].numel() == P + 1
        assert gt["ignore"].dtype == torch.int32 and gt["box"].dtype == torch.float64 and gt["area"].dtype == torch.float64
        assert iou_thr.dtype == torch.float64 and area_rng.dtype == torch.float64 and area_rng.is_contiguous()
        matched = torch.zeros(n, dtype=torch.int64, device=self.device)
        ignored = torch.zeros(n, dtype=torch.int64, device=self.device)
        npig = torch.empty(n_cat, area_rng.shape[0], dtype=torch.int32, device=self.device)
        max_gt = int(gt["max_per_pair"])
        scratch = None
        if self.L.sylph_lvis_match_fits(int(max_det), max_gt) != 1:  # some pair may need it (0), or the entry refuses max_det by name (-1)
            scratch = torch.empty(max(gt["box"].shape[0], 1) * 64, dtype=torch.uint8, device=self.device)
        check(self.L.sylph_lvis_match(self._ctx, n, _ptr(det_rows), P, _ptr(pairs["n"]), n_cat, _ptr(pairs["cat"]), _ptr(pairs["flags"]),
                                      _ptr(pairs["det_off"]), _ptr(gt["box"]), _ptr(gt["area"]), _ptr(gt["ignore"]), _ptr(pairs["gt_off"]), max_gt,
                                      iou_thr.numel(), _ptr(iou_thr), area_rng.shape[0], _ptr(area_rng), int(max_det), _ptr(scratch),
                                      _ptr(matched), _ptr(ignored), _ptr(npig)), "lvis_match")
        return matched, ignored, npig

    def coco_accumulate(self, score: torch.Tensor, rank: torch.Tensor, matched: torch.Tensor, ignored: torch.Tensor, cat_off: torch.Tensor,
                        npig: torch.Tensor, n_thr: int, rec_thr: torch.Tensor, max_dets: torch.Tensor):
        """sylph_coco_accumulate on rows ordered by (category, score descending, image, rank) -> precision [T, R, K, A, M], recall [T, K, A, M],
        scores [T, R, K, A, M] float64 on the device."""
        self._stream()
        n, K, A, M, R = score.numel(), cat_off.numel() - 1, npig.shape[1], max_dets.numel(), rec_thr.numel()
        assert score.dtype == torch.float32 and rank.dtype == torch.int32 and matched.dtype == torch.int64 and ignored.dtype == torch.int64
        assert cat_off.dtype == torch.int32 and npig.dtype == torch.int32 and max_dets.dtype == torch.int32 and rec_thr.dtype == torch.float64
        assert all(t.is_cuda and t.is_contiguous() for t in (score, rank, matched, ignored, cat_off, npig, max_dets, rec_thr))
        precision = torch.empty(n_thr, R, K, A, M, dtype=torch.float64, device=self.device)
        recall = torch.empty(n_thr, K, A, M, dtype=torch.float64, device=self.device)
        scores = torch.empty(n_thr, R, K, A, M, dtype=torch.float64, device=self.device)
        check(self.L.sylph_coco_accumulate(self._ctx, n, _ptr(score), _ptr(rank), _ptr(matched), _ptr(ignored), K, _ptr(cat_off), _ptr(npig),
                                           int(n_thr), R, _ptr(rec_thr), A, M, _ptr(max_dets), _ptr(precision), _ptr(recall), _ptr(scores)),
              "coco_accumulate")
        return precision, recall, scores

    # ---- primitive entries (kernel parity tests) ------------------------------------------------------
    def conv2d(self, x, w, scale=None, shift=None, stride=1, pad=0, relu=False, residual=None):
        self._stream()
        x = x.to(self.device, torch.float32).contiguous()
        B, C, H, W = x.shape
        wh = w.detach().cpu().float().contiguous()
        Cout, _, KH, KW = wh.shape
        Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
        y = torch.empty(B, Cout, Ho, Wo, device=self.device)
        sc = scale.detach().cpu().float().contiguous() if scale is not None else None
        sh = shift.detach().cpu().float().contiguous() if shift is not None else None
        rs = residual.to(self.device, torch.float32).contiguous() if residual is not None else None
        check(self.L.sylph_conv2d(self._ctx, _ptr(x), B, C, H, W, _ptr(wh), Cout, KH, KW, stride, pad, _ptr(sc),
                                  _ptr(sh), int(relu), _ptr(rs), _ptr(y)), "conv2d")
        return y

    def group_norm(self, x, gamma, beta, relu=False):
        self._stream()
        x = x.to(self.device, torch.float32).contiguous()
        B, C, H, W = x.shape
        assert C == 256
        y = torch.empty_like(x)
        g, b = gamma.detach().cpu().float().contiguous(), beta.detach().cpu().float().contiguous()
        check(self.L.sylph_group_norm(self._ctx, _ptr(x), B, H, W, _ptr(g), _ptr(b), int(relu), _ptr(y)), "group_norm")
        return y

    def stem_maxpool(self, x, w, scale, shift):
        """Kernel parity entry (bf16 engines): stem 7x7 s2 + FrozenBN + ReLU and the 3x3 s2 max-pool -> (stem, pool) NCHW fp32."""
        self._stream()
        x = x.to(self.device, torch.float32).contiguous()
        B, C, H, W = x.shape
        assert C == 3
        H2, W2 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        H4, W4 = (H2 - 1) // 2 + 1, (W2 - 1) // 2 + 1
        so = torch.empty(B, 64, H2, W2, device=self.device)
        po = torch.empty(B, 64, H4, W4, device=self.device)
        wh, sc, sh = [t.detach().cpu().float().contiguous() for t in (w, scale, shift)]
        check(self.L.sylph_stem_maxpool(self._ctx, _ptr(x), B, H, W, _ptr(wh), _ptr(sc), _ptr(sh), _ptr(so), _ptr(po)), "stem_maxpool")
        return so, po

    # ---- parity taps (tests) ---------------------------------------------------------------------------
    def set_debug_taps(self, on: bool = True):
        """Keep every tower layer's stored output (call before the first head pass of a batch shape)."""
        check(self.L.sylph_set_debug_taps(self._ctx, int(on)), "set_debug_taps")

    def export_stage(self, stage: int) -> torch.Tensor:
        """res<stage> output of the last backbone pass, (B, C, h, w) fp32 NCHW; C = 256 << (stage - 2), 64 << (stage - 2) for R-18 / R-34,
        24 / 32 / 96 / 320 for MobileNetV2."""
        self._stream()
        B, H, W, _ = self._batch
        h, w = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        for _ in range(stage - 1):
            h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        ch = (24, 32, 96, 320)[stage - 2] if self.sc.mobilenet else (64 if self.sc.resnet_depth in (18, 34) else 256) << (stage - 2)
        out = torch.empty(B, ch, h, w, device=self.device)
        check(self.L.sylph_export_stage(self._ctx, stage, _ptr(out)), "export_stage")
        return out

    def export_tower(self, tower: int, layer: int, with_coef: bool = True):
        """Per level: (conv output (B,256,h,w), GroupNorm coefficients (B,256,2) or None) of one tower layer."""
        self._stream()
        B, H, W, _ = self._batch
        ys, cs = [], []
        for l, (h, w) in enumerate(self.level_shapes(H, W)):
            y = torch.empty(B, 256, h, w, device=self.device)
            cf = torch.empty(B, 256, 2, device=self.device) if with_coef else None
            check(self.L.sylph_export_tower(self._ctx, tower, layer, l, _ptr(y), _ptr(cf)), "export_tower")
            ys.append(y); cs.append(cf)
        return ys, cs

    SUPPORT_STAGES = ("roi", "gn_y", "gn_coef", "layer_out", "conv_out", "context", "mscam", "tokens", "cls_tokens")

    def export_support(self, stage: str, index: int = 0) -> torch.Tensor:
        """One stage output of the last codegen / codegen_classes / codegen_rois call (sylph_export_support; stage names as SUPPORT_STAGES, in the
        order of the SYLPH_SUP_* constants): maps (S, C, 7, 7), GroupNorm coefficients (S, 256, 2), tokens (rows, 256), fp32."""
        self._stream()
        st = self.SUPPORT_STAGES.index(stage)
        n = c_int64(0)
        check(self.L.sylph_support_tap_numel(self._ctx, st, int(index), ctypes.byref(n)), "support_tap_numel")
        out = torch.empty(n.value, device=self.device)
        check(self.L.sylph_export_support(self._ctx, st, int(index), _ptr(out)), "export_support")
        B = self._batch[0] if stage == "context" else self._sup_rows  # per-shot stages: one row per box; the context stays per image
        if stage == "gn_coef":
            return out.view(B, 256, 2)
        if stage in ("tokens", "cls_tokens"):
            return out.view(-1, 256)
        return out.view(B, -1, 7, 7)

    def bottleneck(self, x, ws, scales, shifts, stride=1):
        """One ResNet bottleneck block through the backbone's own launches.  ws / scales / shifts: conv1, conv2, conv3,
        shortcut (or None) weights and folded FrozenBN scale / shift."""
        self._stream()
        x = x.to(self.device, torch.float32).contiguous()
        B, Cin, H, W = x.shape
        mid, cout = ws[0].shape[0], ws[2].shape[0]
        n = 4 if len(ws) > 3 and ws[3] is not None else 3
        keep = [[t.detach().cpu().float().contiguous() for t in lst[:n]] for lst in (ws, scales, shifts)]
        arrs = [(c_void_p * 4)(*([t.data_ptr() for t in lst] + [None] * (4 - n))) for lst in keep]
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        y = torch.empty(B, cout, Ho, Wo, device=self.device)
        check(self.L.sylph_bottleneck(self._ctx, _ptr(x), B, Cin, H, W, stride, mid, cout, arrs[0], arrs[1], arrs[2], _ptr(y)),
              "bottleneck")
        return y

    def bottleneck_even(self, x, ws, scales, shifts):
        """The fused identity block (C 256, mid 64, bf16) through the stride-2-output launch of res2's last block: (B, 256, H/2, W/2), the
        block's output at the even rows and columns.  H and W must be even."""
        self._stream()
        x = x.to(self.device, torch.float32).contiguous()
        B, Cin, H, W = x.shape
        mid, cout = ws[0].shape[0], ws[2].shape[0]
        keep = [[t.detach().cpu().float().contiguous() for t in lst[:3]] for lst in (ws, scales, shifts)]
        arrs = [(c_void_p * 4)(*([t.data_ptr() for t in lst] + [None])) for lst in keep]
        y = torch.empty(B, cout, H // 2, W // 2, device=self.device)
        check(self.L.sylph_bottleneck_even(self._ctx, _ptr(x), B, Cin, H, W, mid, cout, arrs[0], arrs[1], arrs[2], _ptr(y)),
              "bottleneck_even")
        return y

    def res3_pair(self, t2, x, w3, s3, b3, w1, s1, b1):
        """The res3 block-pair launch alone (bf16): y = relu(bn3(w3 t2) + x) (B, 512, H, W) and t1 = relu(bn1(w1 y)) (B, 128, H, W) from
        t2 (B, 128, H, W), x (B, 512, H, W), w3 (512, 128[, 1, 1]), w1 (128, 512[, 1, 1]) and their FrozenBN scale / shift."""
        self._stream()
        t2 = t2.to(self.device, torch.float32).contiguous()
        x = x.to(self.device, torch.float32).contiguous()
        B, _, H, W = x.shape
        host = [t.detach().cpu().float().contiguous() for t in (w3, s3, b3, w1, s1, b1)]
        y = torch.empty(B, 512, H, W, device=self.device)
        t1 = torch.empty(B, 128, H, W, device=self.device)
        check(self.L.sylph_res3_pair(self._ctx, _ptr(t2), _ptr(x), B, H, W, *[_ptr(t) for t in host], _ptr(y), _ptr(t1)), "res3_pair")
        return y, t1

    def bottleneck_grouped(self, x, ws, scales, shifts, stride=1, groups=32):
        """One ResNeXt bottleneck block (conv2 grouped, weight (mid, mid / groups, 3, 3)) through the backbone's own launches."""
        self._stream()
        x = x.to(self.device, torch.float32).contiguous()
        B, Cin, H, W = x.shape
        mid, cout = ws[0].shape[0], ws[2].shape[0]
        n = 4 if len(ws) > 3 and ws[3] is not None else 3
        keep = [[t.detach().cpu().float().contiguous() for t in lst[:n]] for lst in (ws, scales, shifts)]
        arrs = [(c_void_p * 4)(*([t.data_ptr() for t in lst] + [None] * (4 - n))) for lst in keep]
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        y = torch.empty(B, cout, Ho, Wo, device=self.device)
        check(self.L.sylph_bottleneck_grouped(self._ctx, _ptr(x), B, Cin, H, W, stride, mid, cout, groups, arrs[0], arrs[1], arrs[2],
                                              _ptr(y)), "bottleneck_grouped")
        return y

    def group_conv(self, x, w, scale, shift, groups, stride=1, relu=True):
        """One grouped 3x3 conv (pad 1) + FrozenBN scale / shift (+ ReLU) through the ResNeXt conv2 kernel (conv_group.hip)."""
        self._stream()
        x = x.to(self.device, torch.float32).contiguous()
        B, C, H, W = x.shape
        wh = w.detach().cpu().float().contiguous()
        sc, sh = scale.detach().cpu().float().contiguous(), shift.detach().cpu().float().contiguous()
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        y = torch.empty(B, C, Ho, Wo, device=self.device)
        check(self.L.sylph_group_conv(self._ctx, _ptr(x), B, C, H, W, groups, stride, _ptr(wh), _ptr(sc), _ptr(sh), int(relu), _ptr(y)),
              "group_conv")
        return y

    def conv3x3_c64(self, x, w, scale, shift, relu=True, residual=None):
        """One 3x3 stride-1 pad-1 conv 64 -> 64 + FrozenBN scale / shift [+ residual] [+ ReLU] as the res2 convs of R-18 / R-34 launch it
        (conv_rw64.hip in bf16 -- SYLPH_CONV_RW64 0 off / 1 auto / 2 always --, the generic conv route otherwise)."""
        self._stream()
        x = x.to(self.device, torch.float32).contiguous()
        B, C, H, W = x.shape
        assert C == 64 and tuple(w.shape) == (64, 64, 3, 3)
        wh, sc, sh = [t.detach().cpu().float().contiguous() for t in (w, scale, shift)]
        rs = residual.to(self.device, torch.float32).contiguous() if residual is not None else None
        assert rs is None or rs.shape == x.shape
        y = torch.empty_like(x)
        check(self.L.sylph_conv3x3_c64(self._ctx, _ptr(x), B, H, W, _ptr(wh), _ptr(sc), _ptr(sh), int(relu), _ptr(rs), _ptr(y)),
              "conv3x3_c64")
        return y

    def basic_block(self, x, ws, scales, shifts, stride=1):
        """One ResNet BasicBlock (R-18 / R-34) through the backbone's own launches.  ws / scales / shifts: conv1 (cout, Cin, 3, 3),
        conv2 (cout, cout, 3, 3), shortcut (cout, Cin, 1, 1) or None, with their folded FrozenBN scale / shift."""
        self._stream()
        x = x.to(self.device, torch.float32).contiguous()
        B, Cin, H, W = x.shape
        cout = ws[0].shape[0]
        n = 3 if len(ws) > 2 and ws[2] is not None else 2
        keep = [[t.detach().cpu().float().contiguous() for t in lst[:n]] for lst in (ws, scales, shifts)]
        arrs = [(c_void_p * 3)(*([t.data_ptr() for t in lst] + [None] * (3 - n))) for lst in keep]
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        y = torch.empty(B, cout, Ho, Wo, device=self.device)
        check(self.L.sylph_basic_block(self._ctx, _ptr(x), B, Cin, H, W, stride, cout, arrs[0], arrs[1], arrs[2], _ptr(y)), "basic_block")
        return y

    def dwconv3x3(self, x, w, scale, shift, stride=1):
        """One depthwise 3x3 conv (pad 1) as a MobileNetV2 block launches it (conv_dw.hip): relu6(scale * conv(clamp(x, 0, 6)) + shift);
        w (C, 1, 3, 3), C a multiple of 8."""
        self._stream()
        x = x.to(self.device, torch.float32).contiguous()
        B, C, H, W = x.shape
        assert tuple(w.shape) == (C, 1, 3, 3)
        wh, sc, sh = [t.detach().cpu().float().contiguous() for t in (w, scale, shift)]
        y = torch.empty(B, C, (H - 1) // stride + 1, (W - 1) // stride + 1, device=self.device)
        check(self.L.sylph_dwconv3x3(self._ctx, _ptr(x), B, C, H, W, stride, _ptr(wh), _ptr(sc), _ptr(sh), _ptr(y)), "dwconv3x3")
        return y

    def mbv2_padded_channels(self, c: int) -> int:
        """Channels a MobileNetV2 tensor of c channels is stored with (zero pad channels)."""
        return int(self.L.sylph_mbv2_padded_channels(self._ctx, int(c)))

    def mbv2_block(self, x, ws, scales, shifts, stride=1, padded=False):
        """One MobileNetV2 InvertedResidual block through the backbone's own launches.  ws / scales / shifts: expand (6 Cin, Cin, 1, 1) or
        None (t = 1), depthwise (t Cin, 1, 3, 3), project (Cout, t Cin, 1, 1) with their folded FrozenBN scale / shift; the input is added
        when stride == 1 and Cin == Cout.  padded: return the stored pad channels (all zero) too."""
        self._stream()
        x = x.to(self.device, torch.float32).contiguous()
        B, Cin, H, W = x.shape
        t = 1 if ws[0] is None else 6
        cout = ws[2].shape[0]
        assert ws[1].shape[0] == t * Cin and tuple(ws[2].shape[:2]) == (cout, t * Cin)
        keep = [[None if v is None else v.detach().cpu().float().contiguous() for v in lst] for lst in (ws, scales, shifts)]
        arrs = [(c_void_p * 3)(*[None if v is None else v.data_ptr() for v in lst]) for lst in keep]
        cy = self.mbv2_padded_channels(cout) if padded else cout
        y = torch.empty(B, cy, (H - 1) // stride + 1, (W - 1) // stride + 1, device=self.device)
        check(self.L.sylph_mbv2_block(self._ctx, _ptr(x), B, Cin, H, W, t, cout, stride, arrs[0], arrs[1], arrs[2], cy, _ptr(y)), "mbv2_block")
        return y

    def fpn_lateral(self, x, w, bias, top=None):
        """One FPN lateral (1x1 conv + bias [+ nearest-2x upsampled `top`]) through the backbone's own launch."""
        self._stream()
        x = x.to(self.device, torch.float32).contiguous()
        B, C, H, W = x.shape
        wh, bh = w.detach().cpu().float().contiguous(), bias.detach().cpu().float().contiguous()
        tp = top.to(self.device, torch.float32).contiguous() if top is not None else None
        y = torch.empty(B, 256, H, W, device=self.device)
        check(self.L.sylph_fpn_lateral(self._ctx, _ptr(x), B, C, H, W, _ptr(wh), _ptr(bh), _ptr(tp), _ptr(y)), "fpn_lateral")
        return y

    def device_bytes(self) -> int:
        return int(self.L.sylph_device_bytes(self._ctx))

    def bench_conv(self, B, H, W, Cin, Cout, K, stride=1, pad=0, res=False, relu=True, gn=False, iters=10):
        """Kernel micro-benchmark: (ms per launch, TFLOP/s) of one conv layer on random operands."""
        self._stream()
        ms, fl = ctypes.c_float(0), ctypes.c_double(0)
        check(self.L.sylph_bench_conv(self._ctx, B, H, W, Cin, Cout, K, stride, pad, int(res), int(relu), int(gn), iters,
                                      ctypes.byref(ms), ctypes.byref(fl)), "bench_conv")
        return ms.value, fl.value / (ms.value * 1e-3) / 1e12

    def profile_enable(self, on: bool = True):
        check(self.L.sylph_profile_enable(self._ctx, int(on)), "profile_enable")

    def profile_read(self) -> Dict[str, float]:
        """Summed conv-kernel time (HIP events on the launch stream), algorithmic FLOPs, launches -- and the same per kernel
        (`kernels`: name -> {ms, flops, launches})."""
        mx = 64  # distinct kernel names of a step; the list is in order of first launch, so a short buffer would drop the last stages
        names = ctypes.create_string_buffer(mx * 64)
        ms, fl, ln, n = (ctypes.c_double * mx)(), (ctypes.c_double * mx)(), (c_int64 * mx)(), c_int(0)
        check(self.L.sylph_profile_read_kernels(self._ctx, mx, names, ms, fl, ln, ctypes.byref(n)), "profile_read_kernels")
        kern = {}
        for i in range(n.value):
            kern[names.raw[i * 64:(i + 1) * 64].split(b"\0", 1)[0].decode()] = {"ms": ms[i], "flops": fl[i], "launches": int(ln[i])}
        return {"conv_ms": sum(k["ms"] for k in kern.values()), "conv_flops": sum(k["flops"] for k in kern.values()),
                "conv_launches": sum(k["launches"] for k in kern.values()), "kernels": kern}

    def conv_routes(self, max_routes: int = 1024):
        """The route of every conv launch built since the previous call while profiling was on, in build order (consumes them):
        "<kind> <BM>x<BN>[ nbuf<n>][ ks<k>]", kind one of hpipe, igemm_halo, pw, spw, igemm_splitk, igemm."""
        names, n = ctypes.create_string_buffer(max_routes * 64), c_int(0)
        check(self.L.sylph_conv_routes_read(self._ctx, max_routes, names, ctypes.byref(n)), "conv_routes_read")
        return [names.raw[i * 64:(i + 1) * 64].split(b"\0", 1)[0].decode() for i in range(n.value)]
