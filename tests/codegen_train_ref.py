"""Float64 restatement of the code generator's training-mode forward and its hand-written backward (TEST INFRASTRUCTURE).

CodeGeneratorHead.forward_roi_align, training branch (reference code_generator.py:924-1002 with :766-875), on fixed ROI maps:

    per tower layer i (["GN", "ReLU"]):  y_i = conv3x3_pad1(x_i, W_i) + b_i;  x_{i+1} = relu(GroupNorm32(y_i))        per shot
    c[s]  = mean over the 49 positions of conv3x3_pad1(x_L, W_cls) + b_cls;  rb[s] likewise with the bias head (absent: 0)
    code_raw[j], bias_raw[j] = mean over the shots of segment j
    code[j] = conv_scale * l2_normalize(GroupNorm32(code_raw[j]));  bias[j] = bias_scale * bias_raw[j] + prior

`forward` is written with torch.nn.functional so that autograd differentiates it; `backward` is the hand-written gradient the kernels of
csrc/codegen_train.hip implement.  rounding=True rounds where the kernels round -- every conv weight to bf16 at the operand, x_{i+1} to
bf16 where it is stored -- and treats each rounding as the identity in the gradient (straight-through); round_grad=True also rounds
d y_i to bf16 where it enters the data- and weight-gradient products, as the kernels do.
"""
import math
from typing import Dict, List, Sequence

import torch
import torch.nn.functional as F

P = "code_generator.code_generator_head"
GN_EPS = 1e-5


def rbf(t: torch.Tensor) -> torch.Tensor:
    """bf16 round-to-nearest-even of the values, in t's dtype"""
    return t.detach().to(torch.float32).to(torch.bfloat16).to(t.dtype)


def st_round(t: torch.Tensor, on: bool) -> torch.Tensor:
    """the rounded value with the identity as its derivative"""
    return t + (rbf(t) - t.detach()) if on else t


def layout_keys(tower_layers: int, has_bias: bool, post_norm: bool, conv_l2_norm: bool, use_weight_scale: bool = True) -> List[str]:
    """state-dict keys of the trainable tensors, in the order of the flat vector (sylph_codegen_param_layout)"""
    keys = []
    for i in range(tower_layers):
        keys += [f"{P}.support_set_shared_tower.{3 * i}.weight", f"{P}.support_set_shared_tower.{3 * i}.bias",
                 f"{P}.support_set_shared_tower.{3 * i + 1}.weight", f"{P}.support_set_shared_tower.{3 * i + 1}.bias"]
    keys += [f"{P}.support_set_cls_conv.0.weight", f"{P}.support_set_cls_conv.0.bias"]
    if has_bias:
        keys += [f"{P}.support_set_cls_bias.0.weight", f"{P}.support_set_cls_bias.0.bias"]
    if post_norm:
        keys += [f"{P}.post_norm.weight", f"{P}.post_norm.bias"]
    if use_weight_scale and (post_norm or conv_l2_norm):
        keys += [f"{P}.conv_scale.scale"]
    if has_bias:
        keys += [f"{P}.bias_scale.scale"]
    return keys


def prior(prior_prob: float = 0.01) -> float:
    return -math.log((1 - prior_prob) / prior_prob)


def forward(x0: torch.Tensor, sd: Dict[str, torch.Tensor], seg_len: Sequence[int], *, tower_layers: int, has_bias: bool, post_norm: bool,
            conv_l2_norm: bool, use_weight_scale: bool = True, prior_prob: float = 0.01, rounding: bool = False):
    """x0 (M, 256, 7, 7) -> (code (n_seg, 256), bias (n_seg), saved): saved holds every intermediate the backward needs"""
    sv = {"x": [x0], "y": [], "w": [], "seg_len": list(seg_len)}
    x = x0
    for i in range(tower_layers):
        w = st_round(sd[f"{P}.support_set_shared_tower.{3 * i}.weight"], rounding)
        y = F.conv2d(x, w, sd[f"{P}.support_set_shared_tower.{3 * i}.bias"], padding=1)
        x = F.relu(F.group_norm(y, 32, sd[f"{P}.support_set_shared_tower.{3 * i + 1}.weight"], sd[f"{P}.support_set_shared_tower.{3 * i + 1}.bias"], eps=GN_EPS))
        x = st_round(x, rounding)
        sv["w"].append(w); sv["y"].append(y); sv["x"].append(x)
    wc = st_round(sd[f"{P}.support_set_cls_conv.0.weight"], rounding)
    c = F.conv2d(x, wc, sd[f"{P}.support_set_cls_conv.0.bias"], padding=1).mean(dim=(2, 3))
    sv["wc"] = wc; sv["c"] = c
    rb = torch.zeros(x.shape[0], dtype=x.dtype)
    if has_bias:
        wb = st_round(sd[f"{P}.support_set_cls_bias.0.weight"], rounding)
        rb = F.conv2d(x, wb, sd[f"{P}.support_set_cls_bias.0.bias"], padding=1).mean(dim=(2, 3)).reshape(-1)
        sv["wb"] = wb
    sv["rb"] = rb
    code_raw = torch.stack([t.mean(dim=0) for t in torch.split(c, list(seg_len))])
    bias_raw = torch.stack([t.mean() for t in torch.split(rb, list(seg_len))])
    sv["code_raw"] = code_raw; sv["bias_raw"] = bias_raw
    code = code_raw
    if post_norm:
        code = F.group_norm(code, 32, sd[f"{P}.post_norm.weight"], sd[f"{P}.post_norm.bias"], eps=GN_EPS)
    if conv_l2_norm:
        code = F.normalize(code, p=2, dim=1)
    if use_weight_scale and (post_norm or conv_l2_norm):
        code = code * sd[f"{P}.conv_scale.scale"]
    bias = bias_raw * sd[f"{P}.bias_scale.scale"] if has_bias else bias_raw
    bias = bias + prior(prior_prob)
    return code, bias, sv


def gn_backward(g: torch.Tensor, y: torch.Tensor, gamma: torch.Tensor, groups: int = 32):
    """g = d loss / d GroupNorm(y) over (N, C, ...) -> (d y, d gamma, d beta)"""
    N, C = y.shape[:2]
    yg = y.reshape(N, groups, -1)
    mean = yg.mean(dim=2, keepdim=True)
    rstd = 1.0 / torch.sqrt(yg.var(dim=2, unbiased=False, keepdim=True) + GN_EPS)
    xh = ((yg - mean) * rstd).reshape(y.shape)
    red = [0] + list(range(2, y.dim()))
    dgamma = (g * xh).sum(dim=red)
    dbeta = g.sum(dim=red)
    dxh = (g * gamma.reshape([1, C] + [1] * (y.dim() - 2))).reshape(N, groups, -1)
    xhg = xh.reshape(N, groups, -1)
    dy = rstd * (dxh - dxh.mean(dim=2, keepdim=True) - xhg * (dxh * xhg).mean(dim=2, keepdim=True))
    return dy.reshape(y.shape), dgamma, dbeta


def backward(sd: Dict[str, torch.Tensor], sv, g_code: torch.Tensor, g_bias: torch.Tensor, *, tower_layers: int, has_bias: bool, post_norm: bool,
             conv_l2_norm: bool, use_weight_scale: bool = True, round_grad: bool = False, stages: Dict[str, torch.Tensor] = None):
    """gradient of sum(code * g_code) + sum(bias * g_bias) with respect to every trainable tensor, as a dict by state-dict key; `stages`,
    when given, receives d code_raw, d c, d x_i, d y_i"""
    grads = {}
    seg_len = sv["seg_len"]
    v0 = sv["code_raw"]
    n_seg = v0.shape[0]
    # the tail, per class
    v1 = v0
    if post_norm:
        v1 = F.group_norm(v0, 32, sd[f"{P}.post_norm.weight"], sd[f"{P}.post_norm.bias"], eps=GN_EPS)
    nrm = v1.norm(dim=1, keepdim=True).clamp_min(1e-12)
    v2 = v1 / nrm if conv_l2_norm else v1
    has_cs = use_weight_scale and (post_norm or conv_l2_norm)
    cs = sd[f"{P}.conv_scale.scale"] if has_cs else torch.ones(1, dtype=v0.dtype)
    if has_cs:
        grads[f"{P}.conv_scale.scale"] = (g_code * v2).sum().reshape(1)
    dv2 = g_code * cs
    dv1 = (dv2 - v2 * (dv2 * v2).sum(dim=1, keepdim=True)) / nrm if conv_l2_norm else dv2
    dv0 = dv1
    if post_norm:
        dv0, dg, db = gn_backward(dv1, v0, sd[f"{P}.post_norm.weight"])
        grads[f"{P}.post_norm.weight"] = dg
        grads[f"{P}.post_norm.bias"] = db
    d_bias_raw = torch.zeros(n_seg, dtype=v0.dtype)
    if has_bias:
        grads[f"{P}.bias_scale.scale"] = (g_bias * sv["bias_raw"]).sum().reshape(1)
        d_bias_raw = g_bias * sd[f"{P}.bias_scale.scale"]
    lens = torch.tensor(seg_len, dtype=v0.dtype)
    dc = torch.repeat_interleave(dv0 / lens[:, None], torch.tensor(seg_len), dim=0)
    drb = torch.repeat_interleave(d_bias_raw / lens, torch.tensor(seg_len), dim=0)
    # the heads: the pooled conv's output gradient is d c / 49 at every position
    xL = sv["x"][-1]
    M = xL.shape[0]
    gmap = (dc / 49.0)[:, :, None, None].expand(M, 256, 7, 7).contiguous()
    grads[f"{P}.support_set_cls_conv.0.weight"] = torch.nn.grad.conv2d_weight(xL, sv["wc"].shape, gmap, padding=1)
    grads[f"{P}.support_set_cls_conv.0.bias"] = dc.sum(dim=0)
    dx = torch.nn.grad.conv2d_input(xL.shape, sv["wc"].detach(), gmap, padding=1) if tower_layers else None
    if has_bias:
        bmap = (drb / 49.0)[:, None, None, None].expand(M, 1, 7, 7).contiguous()
        grads[f"{P}.support_set_cls_bias.0.weight"] = torch.nn.grad.conv2d_weight(xL, sv["wb"].shape, bmap, padding=1)
        grads[f"{P}.support_set_cls_bias.0.bias"] = drb.sum().reshape(1)
        if tower_layers:
            dx = dx + torch.nn.grad.conv2d_input(xL.shape, sv["wb"].detach(), bmap, padding=1)
    if stages is not None:
        stages.update({"d_code_raw": dv0, "d_bias_raw": d_bias_raw, "d_c": dc, "d_rb": drb})
        if tower_layers:
            stages[f"d_x{tower_layers}"] = dx
    for i in range(tower_layers - 1, -1, -1):
        g = dx * (sv["x"][i + 1] > 0).to(dx.dtype)
        dy, dg, db = gn_backward(g, sv["y"][i], sd[f"{P}.support_set_shared_tower.{3 * i + 1}.weight"])
        grads[f"{P}.support_set_shared_tower.{3 * i + 1}.weight"] = dg
        grads[f"{P}.support_set_shared_tower.{3 * i + 1}.bias"] = db
        grads[f"{P}.support_set_shared_tower.{3 * i}.bias"] = dy.sum(dim=(0, 2, 3))
        dyo = rbf(dy) if round_grad else dy
        grads[f"{P}.support_set_shared_tower.{3 * i}.weight"] = torch.nn.grad.conv2d_weight(sv["x"][i].detach(), sv["w"][i].shape, dyo, padding=1)
        if stages is not None:
            stages[f"d_y{i}"] = dy
        if i > 0:
            dx = torch.nn.grad.conv2d_input(sv["x"][i].shape, sv["w"][i].detach(), dyo, padding=1)
            if stages is not None:
                stages[f"d_x{i}"] = dx
    return {k: v.detach() for k, v in grads.items()}


def flat(d: Dict[str, torch.Tensor], keys: Sequence[str]) -> torch.Tensor:
    return torch.cat([d[k].reshape(-1) for k in keys])


def unflat(v: torch.Tensor, keys: Sequence[str], like: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    out, o = {}, 0
    for k in keys:
        n = like[k].numel()
        out[k] = v[o:o + n].reshape(like[k].shape)
        o += n
    return out


def rows_to_maps(rows: torch.Tensor) -> torch.Tensor:
    """(M, 49, 256) position-major rows -> (M, 256, 7, 7)"""
    return rows.reshape(rows.shape[0], 7, 7, 256).permute(0, 3, 1, 2).contiguous()


def loop_ref(maps: torch.Tensor, sd: Dict[str, torch.Tensor], episodes, step_inputs, *, lr: float, momentum: float = 0.9, weight_decay: float = 1e-4,
             clip_norm: float = 1.0, alpha: float = 0.25, gamma: float = 2.0, **kw) -> List[float]:
    """train_code_generator restated in float64 with the kernels' roundings: episodes[t] = (idx, seg_len) of step t, step_inputs[t] the
    step's records as (xn (rows, 256) operand values of the cls tower, labels (rows,) renumbered to the episode) -> the loss of every step"""
    import finetune_ref as FR
    keys = layout_keys(kw["tower_layers"], kw["has_bias"], kw["post_norm"], kw["conv_l2_norm"])
    p = {k: sd[k].double().clone() for k in keys}
    buf = None
    losses = []
    for (idx, seg_len), recs in zip(episodes, step_inputs):
        code, bias, sv = forward(maps[torch.tensor(idx)], p, seg_len, rounding=True, **kw)
        out = [FR.cls_grad_ref(xn, lab, code.float(), bias.float(), alpha, gamma) for xn, lab in recs]
        npos = max(sum(int((lab >= 0).sum()) for _, lab in recs), 1)
        losses.append(float(sum(o["loss"] for o in out)) / npos)
        grads = backward(p, sv, sum(o["gw"] for o in out) / npos, sum(o["gb"] for o in out) / npos, **kw)
        g = flat(grads, keys)
        g = g * min(1.0, clip_norm / (float(g.norm()) + 1e-6)) if clip_norm is not None else g
        v = flat(p, keys)
        d = g + weight_decay * v
        buf = d.clone() if buf is None else momentum * buf + d
        p = unflat(v - lr * buf, keys, p)
    return losses
