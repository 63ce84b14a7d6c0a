"""Oracle, bf16-storage mode: the same layer graph as oracle/backbone.py + oracle/head.py, but every tensor the
HIP throughput path STORES as bf16 is rounded to bf16 at the same point (round-to-nearest-even, like
v_cvt_pk_bf16_f32), with fp32 accumulation and fp32 epilogue arithmetic in between.  TEST INFRASTRUCTURE
(tests/, smoke(), bench.py's parity leg only); torch CPU.

With identical operands a HIP kernel and this restatement then round the SAME fp32 value up to accumulation
order (~1e-6 relative), so per-kernel outputs agree bit for bit except where that value sits on a bf16
rounding boundary (a 1-ulp flip, 2^-8 relative): the bf16 production kernels can be pinned to ulps instead
of to a cosine.

Storage points restated here:
  * network input after (x - mean) / std                          -> bf16   (preprocess_kernel)
  * every conv epilogue: acc * bn_scale + bn_shift (one fma) [+ residual] [ReLU] -> bf16
    (conv_igemm / conv_pw / conv_hpipe / bottleneck64[p] / stem_pool), weights bf16, un-scaled
  * a block with a projection shortcut: conv3 and the shortcut are ONE GEMM over K = [t2 | x]; the two
    FrozenBN scales are folded into the weights in fp32 BEFORE the bf16 cast, the shifts are summed
    (api_weights.hip make_c3sc)
  * FPN lateral (+ nearest-2x top-down), output convs, P6, relu(P6), P7: bias epilogue -> bf16
  * FCOS towers: conv + bias -> bf16 (stored PRE-GroupNorm); GroupNorm statistics from the fp32 epilogue
    values (before rounding); the consumer applies x <- bf16(relu(fma(a, x, b))) to the stored bf16 values
  * class-conditional conv: bf16 normalised features x bf16 codes, fp32 logits + bias
  * bbox/ctrness/iou prediction conv: bf16 normalised features x bf16 weights, fp32, + bias, Scale, ReLU

Support path (api_codegen.hip build_support / build_support_roienc, add_conv_gn in api_conv.hip, codegen.hip, roi_encoder.hip):
  * ROIAlign: fp32 sum of the bilinear samples of the bf16 pyramid, divided by the count -> bf16   (roi_align_kernel<bf16_t>)
  * tower layer with GroupNorm: conv + bias, bf16 weights -> bf16 stored PRE-GroupNorm; statistics from the fp32 epilogue values;
    the in-place apply x <- bf16(act(fma(a, x_stored, b)))                          (gn_apply_partials_kernel, as the FCOS towers)
  * tower layer without GroupNorm: bf16(act(conv + bias))
  * cls / bias / shot-weight / class-scale convs: bf16 operands, fp32 outputs (out_f32); the tail -- mean over the 49 positions,
    uniform or softmax shot weights, BIAS_L2_NORM -- and normalize_codes are fp32                      (codegen_tail_kernel)
  * ROIEncoder: context fp32 from the bf16 pyramid; box_pooler conv + GroupNorm as a tower layer; MS-CAM gate fp32,
    x <- bf16(x * sigmoid(z)); tokenizer convs (no bias) + GroupNorm as tower layers; the first tokenizer FC reads the bf16
    activations (position-major, with its weight columns permuted to match at load: the same sum as the reference's channel-major
    flatten); everything after it -- FCs, encoder layers, class tokens, heads -- fp32

Reference ops: the same as oracle/backbone.py and oracle/head.py (detectron2 ResNet/FPN at the call sites
sylph/modeling/meta_arch/meta_one_stage_detector.py:181,273; sylph/modeling/meta_fcos/fcos.py:72-122,582-667), oracle/codegen.py
and oracle/roi_encoder.py for the support path.

Against the reference goldens (fp32 reference on bf16-representable pyramids) this restatement differs by its roundings only.  Each
bf16 store adds a relative error of at most 2^-9 per element; the convs, GroupNorms and FCs between the stores keep the relative
L2 size of such an error (He-initialised weights, normalised activations), and the pools and token means only average it.  A path
with k stores is therefore within relative L2 k * 2^-9 of the reference: k = 5 for the two-layer code generator (ROI, two
pre-GroupNorm outputs, two applied outputs), k = 8 for the ROIEncoder (ROI, box_pooler y and x, MS-CAM output, two tokenizer y
and x) -- tests/test_oracle_bf16.py holds the codes to that.
"""
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import backbone as _bb
from .head import GN_EPS, GN_GROUPS, HEAD_PREFIX


def r(t: torch.Tensor) -> torch.Tensor:
    """Round to bf16 (nearest even) and widen back: the value a bf16 store + load yields."""
    return t.to(torch.bfloat16).to(torch.float32)


def fma(x: torch.Tensor, a, b) -> torch.Tensor:
    """fp32 fused multiply-add x * a + b (one rounding): the product of two fp32 values is exact in float64."""
    a = a if torch.is_tensor(a) else torch.tensor(a, dtype=torch.float32)
    b = b if torch.is_tensor(b) else torch.tensor(b, dtype=torch.float32)
    return (x.double() * a.double() + b.double()).float()


def _cv(v: Optional[torch.Tensor]):
    return v.view(1, -1, 1, 1) if v is not None else None


def conv_epilogue(x_bf: torch.Tensor, w: torch.Tensor, scale: Optional[torch.Tensor], shift: Optional[torch.Tensor],
                  stride: int = 1, padding: int = 0, relu: bool = False, res_bf: Optional[torch.Tensor] = None):
    """One conv launch: bf16 operands, fp32 accumulate, v = fma(acc, scale, shift) (+ residual) (ReLU).
    Returns (v fp32 before the store, r(v) as stored)."""
    acc = F.conv2d(x_bf, r(w), None, stride=stride, padding=padding)
    sc = _cv(scale) if scale is not None else 1.0
    sh = _cv(shift) if shift is not None else 0.0
    v = fma(acc, sc, sh)
    if res_bf is not None:
        v = v + res_bf
    if relu:
        v = F.relu(v)
    return v, r(v)


def preprocess(images: Sequence[torch.Tensor]):
    x, sizes = _bb.preprocess(images)
    return r(x), sizes


def stem_pool(x_bf, sd, prefix="backbone.bottom_up"):
    sc, sh = _bb.bn_scale_shift(sd, prefix + ".stem.conv1.norm")
    _, y = conv_epilogue(x_bf, sd[prefix + ".stem.conv1.weight"], sc, sh, stride=2, padding=3, relu=True)
    return F.max_pool2d(y, kernel_size=3, stride=2, padding=1)


def bottleneck_params(sd, prefix, has_shortcut):
    """-> (ws, scales, shifts) of conv1, conv2, conv3, shortcut (None for an identity block)."""
    names = ["conv1", "conv2", "conv3"] + (["shortcut"] if has_shortcut else [])
    ws = [sd[f"{prefix}.{n}.weight"] for n in names]
    ss = [_bb.bn_scale_shift(sd, f"{prefix}.{n}.norm") for n in names]
    return ws, [s[0] for s in ss], [s[1] for s in ss]


def bottleneck(x_bf, ws, scales, shifts, stride, stride_in_1x1=True):
    """One block as the HIP graph computes it (t1, t2 stored bf16; projection folded into conv3's GEMM)."""
    s1, s3 = (stride, 1) if stride_in_1x1 else (1, stride)
    _, t1 = conv_epilogue(x_bf, ws[0], scales[0], shifts[0], stride=s1, relu=True)
    _, t2 = conv_epilogue(t1, ws[1], scales[1], shifts[1], stride=s3, padding=1, relu=True)
    if len(ws) > 3 and ws[3] is not None:
        w3f = r(ws[2] * scales[2].view(-1, 1, 1, 1))
        wsf = r(ws[3] * scales[3].view(-1, 1, 1, 1))
        acc = F.conv2d(t2, w3f) + F.conv2d(x_bf, wsf, stride=stride)
        v = F.relu(acc + (shifts[2] + shifts[3]).view(1, -1, 1, 1))
        return r(v)
    _, y = conv_epilogue(t2, ws[2], scales[2], shifts[2], relu=True, res_bf=x_bf)
    return y


def resnet(x_bf, sd, depth=50, prefix="backbone.bottom_up", start_stage=2, x_stage=None):
    """bf16-storage ResNet bottom-up.  start_stage > 2 with x_stage: start from a given res<start_stage - 1> output
    (stage-wise comparison against sylph_export_stage).  Returns {res2..res5}."""
    x = stem_pool(x_bf, sd, prefix) if start_stage == 2 else x_stage
    outs = {}
    for si, nblocks in enumerate(_bb.STAGE_BLOCKS[depth]):
        stage = si + 2
        if stage < start_stage:
            continue
        for bi in range(nblocks):
            stride = 2 if (bi == 0 and stage > 2) else 1
            ws, ss, hs = bottleneck_params(sd, f"{prefix}.res{stage}.{bi}", bi == 0)
            x = bottleneck(x, ws, ss, hs, stride)
        outs[f"res{stage}"] = x
    return outs


def fpn(feats: Dict[str, torch.Tensor], sd, prefix="backbone"):
    def conv(x, name, stride=1, padding=0, res=None):
        return conv_epilogue(x, sd[f"{prefix}.{name}.weight"], None, sd[f"{prefix}.{name}.bias"], stride=stride,
                             padding=padding, res_bf=res)[1]
    prev = conv(feats["res5"], "fpn_lateral5")
    out = {"p5": conv(prev, "fpn_output5", padding=1)}
    for stage in (4, 3):
        top_down = F.interpolate(prev, scale_factor=2.0, mode="nearest")
        prev = conv(feats[f"res{stage}"], f"fpn_lateral{stage}", res=top_down)
        out[f"p{stage}"] = conv(prev, f"fpn_output{stage}", padding=1)
    p6 = conv(out["p5"], "top_block.p6", stride=2, padding=1)
    out["p6"] = p6
    out["p7"] = conv(F.relu(p6), "top_block.p7", stride=2, padding=1)
    return out


def backbone_fpn(x_bf, sd, depth=50) -> List[torch.Tensor]:
    f = fpn(resnet(x_bf, sd, depth), sd)
    return [f[k] for k in ("p3", "p4", "p5", "p6", "p7")]


# ---- head -------------------------------------------------------------------------------------------
def gn_coef(v: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor) -> torch.Tensor:
    """GroupNorm(32) statistics of the fp32 epilogue values v (B,256,h,w) -> (B,256,2) coefficients (a, b) with
    GN(x) = a * x + b (elementwise.hip gn_finalize_partials_kernel: float64 merge; gn_coef_kernel: fp32)."""
    B, C = v.shape[0], v.shape[1]
    g = v.double().reshape(B, GN_GROUPS, -1)
    mean = g.mean(dim=2)
    var = g.var(dim=2, unbiased=False)
    rstd = (1.0 / torch.sqrt(var + GN_EPS)).float().repeat_interleave(C // GN_GROUPS, dim=1)
    mean = mean.float().repeat_interleave(C // GN_GROUPS, dim=1)
    a = rstd * gamma.view(1, -1)
    b = beta.view(1, -1) - mean * a
    return torch.stack([a, b], dim=2)


def gn_apply(y_bf: torch.Tensor, coef: torch.Tensor, relu: bool = True) -> torch.Tensor:
    """x <- bf16(relu(fma(a, y, b))): what the consumer of a tower layer feeds its MFMAs."""
    a = coef[:, :, 0].reshape(coef.shape[0], -1, 1, 1)
    b = coef[:, :, 1].reshape(coef.shape[0], -1, 1, 1)
    v = fma(y_bf, a, b)
    return r(F.relu(v) if relu else v)


def tower_layer(x_bf, sd, prefix, i):
    """conv3x3 + bias of tower layer i -> (fp32 epilogue values, stored bf16 values, GroupNorm coefficients)."""
    v, y = conv_epilogue(x_bf, sd[f"{prefix}.{3 * i}.weight"], None, sd[f"{prefix}.{3 * i}.bias"], padding=1)
    return v, y, gn_coef(v, sd[f"{prefix}.{3 * i + 1}.weight"], sd[f"{prefix}.{3 * i + 1}.bias"])


def tower(x_bf, sd, prefix, num_convs=4):
    """-> normalised bf16 features of the last layer (the MFMA operand of the prediction passes)."""
    for i in range(num_convs):
        _, y, cf = tower_layer(x_bf, sd, prefix, i)
        x_bf = gn_apply(y, cf)
    return x_bf


def cls_logits(xn_bf, w, b):
    """Class-conditional 1x1 conv: bf16 codes (pack_codes_kernel), fp32 accumulate, + bias."""
    return F.conv2d(xn_bf, r(w), None) + (_cv(b) if b is not None else 0.0)


def predictions(xn_bf, sd, level, use_scale=True, prefix=HEAD_PREFIX):
    """-> reg (B,4,h,w) = relu(scale_l * (bbox_pred + bias)), ctrness, iou_overlap (fp32)."""
    reg = F.conv2d(xn_bf, r(sd[f"{prefix}.bbox_pred.weight"]), None, padding=1) + _cv(sd[f"{prefix}.bbox_pred.bias"])
    if use_scale:
        reg = reg * sd[f"{prefix}.scales.{level}.scale"]
    ctr = F.conv2d(xn_bf, r(sd[f"{prefix}.ctrness.weight"]), None, padding=1) + _cv(sd[f"{prefix}.ctrness.bias"])
    iou = F.conv2d(xn_bf, r(sd[f"{prefix}.iou_overlap.weight"]), None, padding=1) + _cv(sd[f"{prefix}.iou_overlap.bias"])
    return F.relu(reg), ctr, iou


def fcos_head(features_bf: List[torch.Tensor], sd, class_codes, num_convs=4, use_scale=True, prefix=HEAD_PREFIX):
    w, b = class_codes["cls_conv"], class_codes["cls_bias"]
    logits, regs, ctrs, ious = [], [], [], []
    for level, feat in enumerate(features_bf):
        ct = tower(feat, sd, f"{prefix}.cls_tower", num_convs)
        bt = tower(feat, sd, f"{prefix}.bbox_tower", num_convs)
        logits.append(cls_logits(ct, w, b))
        reg, ctr, iou = predictions(bt, sd, level, use_scale, prefix)
        regs.append(reg); ctrs.append(ctr); ious.append(iou)
    return logits, regs, ctrs, ious


def forward_instances(images, class_codes, sd, depth=50, post_nms_topk=100, **decode_kw):
    """bf16-storage twin of oracle.episode.forward_instances (decode itself is fp32 in both paths)."""
    from . import decode as _dec
    x, sizes = preprocess(images)
    feats = backbone_fpn(x, sd, depth)
    logits, regs, ctrs, ious = fcos_head(feats, sd, class_codes)
    props = _dec.predict_proposals(logits, regs, ctrs, ious, post_nms_topk=post_nms_topk, **decode_kw)
    return [_dec.detector_postprocess(p, sizes[i], sizes[i][0], sizes[i][1]) for i, p in enumerate(props)]


# ---- support path ------------------------------------------------------------------------------------------
def roi_pool(features_bf: List[torch.Tensor], boxes: torch.Tensor, strides=(8, 16, 32, 64, 128)) -> torch.Tensor:
    """ROIAlignV2 of the bf16 pyramid, one box per image: fp32 sample sum / count, one bf16 rounding -> (S,256,7,7)."""
    from .roi_align import roi_pooler
    return r(roi_pooler(features_bf, boxes, strides, out_size=7))


def support_layer(x_bf, w, b, gamma=None, beta=None, act="ReLU"):
    """One 7x7 support conv layer (pad 1) -> (fp32 epilogue v, stored bf16 y, GroupNorm (a, b) or None, output x).
    With GroupNorm: y is stored pre-GroupNorm and x = bf16(act(fma(a, y, b))); without: x = y = bf16(act(v))."""
    v = F.conv2d(x_bf, r(w), None, padding=1)
    if b is not None:
        v = v + _cv(b)
    if gamma is None:
        v = F.relu(v) if act == "ReLU" else torch.tanh(v) if act == "Tanh" else v
        return v, r(v), None, r(v)
    cf = gn_coef(v, gamma, beta)
    y = r(v)
    return v, y, cf, gn_apply(y, cf, act == "ReLU")


def support_conv_f32(x_bf, w, b):
    """cls / bias / shot-weight / class-scale conv: bf16 operands, fp32 output + bias."""
    return F.conv2d(x_bf, r(w), None, padding=1) + _cv(b)


def codegen_tail(conv_out, bias_map, shots, weight_map=None, scale_map=None, bias_l2_norm=False):
    """codegen_tail_kernel in fp32: per class of `shots` consecutive images, the 49-position means of the conv outputs combined with
    uniform (1/shots) or softmax(pooled shot-weight logits) weights -> (codes (classes, 257): cls_conv | cls_bias, cls_weight_norm
    (classes,) or None)."""
    S = conv_out.shape[0]
    ncls = S // shots
    pooled = conv_out.flatten(2).mean(dim=2).view(ncls, shots, -1)
    if weight_map is not None:
        w = torch.softmax(weight_map.flatten(1).mean(dim=1).view(ncls, shots), dim=1)
    else:
        w = torch.full((ncls, shots), 1.0 / shots)
    codes = torch.zeros(ncls, conv_out.shape[1] + 1)
    codes[:, :-1] = (w.unsqueeze(2) * pooled).sum(dim=1)
    if bias_map is not None:
        bm = bias_map.flatten(1)
        if bias_l2_norm:
            bm = F.normalize(bm, p=2, dim=1)
        codes[:, -1] = (w * bm.mean(dim=1).view(ncls, shots)).sum(dim=1)
    wn = None
    if scale_map is not None:
        wn = (w * scale_map.flatten(1).mean(dim=1).view(ncls, shots)).sum(dim=1)
    return codes, wn


def codegen_support(features_bf, boxes, sd, shots, spec=None, weight_layer=False, scale_layer=False, bias_l2_norm=False):
    """The code generator's support path as the HIP graph stores it -> {"roi", "layers": [(v, y, coef, x)], "conv_out", "aux":
    {name: fp32 map}, "codes" (classes, 257), "wnorm"}."""
    from .codegen import CG_PREFIX
    p = f"{CG_PREFIX}.support_set_shared_tower"
    spec = spec if spec is not None else [["GN", "ReLU"]] * 2
    out = {"roi": roi_pool(features_bf, boxes), "layers": []}
    x, idx = out["roi"], 0
    for norm, act in spec:
        w, b = sd[f"{p}.{idx}.weight"], sd[f"{p}.{idx}.bias"]
        idx += 1
        g = bt = None
        if norm == "GN":
            g, bt = sd[f"{p}.{idx}.weight"], sd[f"{p}.{idx}.bias"]
            idx += 1
        if act in ("ReLU", "Tanh"):
            idx += 1
        lay = support_layer(x, w, b, g, bt, act)
        out["layers"].append(lay)
        x = lay[3]
    conv = lambda name: support_conv_f32(x, sd[f"{CG_PREFIX}.{name}.0.weight"], sd[f"{CG_PREFIX}.{name}.0.bias"])
    out["conv_out"] = conv("support_set_cls_conv")
    out["aux"] = {"bias": conv("support_set_cls_bias")}
    if weight_layer:
        out["aux"]["weight"] = conv("support_set_cls_weight")
    if scale_layer:
        out["aux"]["scale"] = conv("support_set_cls_scale")
    out["codes"], out["wnorm"] = codegen_tail(out["conv_out"], out["aux"]["bias"], shots, out["aux"].get("weight"),
                                              out["aux"].get("scale"), bias_l2_norm)
    return out


def roienc_context(features_bf):
    """adaptive_context_kernel: mean over the levels of the 7x7 adaptive average pools of the bf16 pyramid, fp32."""
    return torch.stack([F.adaptive_avg_pool2d(f, (7, 7)) for f in features_bf]).mean(dim=0)


def mscam(x_bf, context, sd, prefix="code_generator.box_pooler.context_attention_module"):
    """MS-CAM gate of the box_pooler output: fp32 gate from the context, x <- bf16(x * sigmoid(z))."""
    from .roi_encoder import ms_cam
    return r(ms_cam(x_bf, context, sd, prefix))


def tokenizer_fc(x_bf, sd, tok_fcs=2, position_major=False):
    """Tokenizer FC stack on the bf16 (S,256,7,7) activations -> (S, fc_dim) fp32.  The first FC reads the activations in the HIP
    layout (position-major) with its weight columns permuted to match, i.e. the reference's channel-major sum;
    position_major=True pairs the position-major activations with the UN-permuted weights (a wrong kernel)."""
    t = x_bf.permute(0, 2, 3, 1).flatten(1) if position_major else x_bf.flatten(1)
    for k in range(tok_fcs):
        t = F.relu(F.linear(t, sd[f"code_generator.tokenizer.fc{k + 1}.weight"], sd[f"code_generator.tokenizer.fc{k + 1}.bias"]))
    return t


def encoder_layer(tokens, sd, l, nhead=8):
    """One encoder layer on (S, E) tokens, each its own length-1 sequence (a class never attends to another one), fp32."""
    from .roi_encoder import encoder_layer as _enc
    return _enc(tokens.unsqueeze(0), sd, f"code_generator.transformer_encoder.layers.{l}", nhead)[0]


def roienc_heads(cls_tok, sd, head_fcs=2, prior_prob=0.01):
    """weight / bias heads on the class tokens (classes, E) -> codes (classes, 257), fp32."""
    import math

    def head(t, name):
        for i in range(head_fcs):
            t = F.linear(t, sd[f"code_generator.{name}.fc{i + 1}.weight"], sd[f"code_generator.{name}.fc{i + 1}.bias"])
            t = F.relu(t) if i < head_fcs - 1 else t
        return t
    w, b = head(cls_tok, "weight_head"), head(cls_tok, "bias_head")
    return torch.cat([w, b - math.log((1 - prior_prob) / prior_prob)], dim=1)


def roi_encoder_support(features_bf, boxes, sd, shots, tok_convs=2, tok_fcs=2, layers=2, nhead=8, head_fcs=2):
    """The ROIEncoder support path as the HIP graph stores it -> {"roi", "context", "layers": [(v, y, coef, x)] (box_pooler, then
    the tokenizer convs; layers[0]'s x is BEFORE the MS-CAM gate), "mscam", "tokens": [after the FC stack, after each encoder
    layer], "cls_tokens", "codes" (classes, 257)}."""
    P = "code_generator"
    out = {"roi": roi_pool(features_bf, boxes), "context": roienc_context(features_bf)}
    bp = f"{P}.box_pooler.conv"
    out["layers"] = [support_layer(out["roi"], sd[f"{bp}.0.weight"], sd[f"{bp}.0.bias"], sd[f"{bp}.1.weight"], sd[f"{bp}.1.bias"])]
    x = out["mscam"] = mscam(out["layers"][0][3], out["context"], sd)
    for k in range(tok_convs):
        t = f"{P}.tokenizer.conv{k + 1}"
        out["layers"].append(support_layer(x, sd[f"{t}.weight"], None, sd[f"{t}.norm.weight"], sd[f"{t}.norm.bias"]))
        x = out["layers"][-1][3]
    tok = tokenizer_fc(x, sd, tok_fcs)
    out["tokens"] = [tok]
    for l in range(layers):
        tok = encoder_layer(tok, sd, l, nhead)
        out["tokens"].append(tok)
    out["cls_tokens"] = tok.view(-1, shots, tok.shape[-1]).mean(dim=1)
    out["codes"] = roienc_heads(out["cls_tokens"], sd, head_fcs)
    return out


def ulp_report(got: torch.Tensor, want: torch.Tensor) -> Tuple[float, float]:
    """(fraction of elements that are not bit-identical, worst |difference| in units of the bf16 spacing at that
    magnitude).  Both tensors hold bf16-representable values."""
    diff = (got - want).abs()
    mag = torch.maximum(got.abs(), want.abs()).clamp_min(2.0 ** -126)
    ulp = torch.exp2(torch.floor(torch.log2(mag)) - 7)   # spacing of bf16 (8 significant bits) at that binade
    return float((diff > 0).float().mean()), float((diff / ulp).max())
