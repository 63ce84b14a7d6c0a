"""Float64 GroupNorm statistics, crafted tower layers with a prescribed distribution per output group, and the displacement metric
the GroupNorm statistics tests hold the kernels to (tests/test_gn_statistics_cpu.py, tests/test_gn_statistics_gpu.py).

The GroupNorm statistics of a tower layer come out of conv epilogues in fp32 (three schemes: conv_hpipe.hip, conv_igemm.hip /
conv_deform.hip through gn_tile_reduce, gn_stats_kernel), are merged in fp64 and become per-channel coefficients (a, b) with
y = relu(a x + b).  On randn data the group mean sits on every scheme's pivot and every tile has the same mean, so neither the
distance of the mean from the pivot nor the between-tile term of the merges is exercised.  The crafted layer below gives each of the
32 output groups of ONE conv launch its own distribution: offset groups (mean R sigma away from the conv bias), step groups (left and
right half of every map 16 sigma apart: the between-tile term dominates), zero-variance and constant-per-channel groups, a group with
one huge outlier, and plain controls.

Displacement: for one (segment, channel) with reference mean m*, s* = sqrt(var* + eps), a* = gamma / s*, b* = beta - m* a*,
    disp = max over x in {m* - 4 s*, m* + 4 s*} of |(a - a*) x + (b - b*)|:
how far the kernel's coefficients move a normalised value of that channel.  Bound, per channel (never against a tensor maximum):
    tol_mode + 8 * 2^-24 * (|a* m*| + |a*| 4 s* + |beta|),
the second term being the rounding of fp32 a, b and of the affine form itself (no algorithm avoids it); tol_mode = 2^-10 in bf16 (an
eighth of a bf16 ulp at 1.0, below what storage rounding does to the operand) and 1e-4 in f32 / f32s (the project's rule for fp32
outputs).  The displacement is affine in x, so an element further than 4 s* from the mean is allowed the bound times
|x - m*| / (4 s*)."""
import math

import torch
import torch.nn.functional as F

GN_EPS = 1e-5
GROUPS = 32
U32 = 2.0 ** -24
TOL_MODE = {"bf16": 2.0 ** -10, "f32": 1e-4, "f32s": 1e-4}

# group index -> (kind, R = D / sigma, A / sigma); sigma = 1 by construction
LAYOUT = ([("offset", r, 0.0) for r in (0.0, 4.0, 16.0, 64.0, 256.0, 1024.0)] + [("step", 0.0, 8.0), ("step", 64.0, 8.0)]
          + [("zerovar", 0.0, 0.0), ("zerovar", -1000.0, 0.0), ("constch", 0.0, 0.0), ("outlier", 0.0, 0.0), ("purestep", 0.0, 8.0)]
          + [("control", 0.0, 0.0)] * 19)
STEP_ONLY_LAYOUT = [("step", 0.0, 8.0), ("step", 64.0, 8.0)] + [("control", 0.0, 0.0)] * 30  # the finalizer-tail case
# the pivot rule of conv_hpipe samples a patch's first position: groups whose eight channels share R sigma at position (0, 0) of every map only
CORNER_LAYOUT = [("corner", 64.0, 0.0), ("corner", 1024.0, 0.0), ("outlier", 0.0, 0.0)] + [("control", 0.0, 0.0)] * 29
SUPPORT_LAYOUT = [lay if lay[0] in ("offset", "zerovar") else ("control", 0.0, 0.0) for lay in LAYOUT]  # 49-row segments: no clean step
G_ZERO, G_PURESTEP = 8, 12  # the zero-variance (bias 0) and the noise-free step group of LAYOUT
CONSTCH_BIASES = [-3.0, -1.5, -0.5, 0.0, 0.25, 1.0, 2.0, 4.0]
OUTLIER = 2.0 ** 12


def groups_of(layout, kind):
    return [g for g, lay in enumerate(layout) if lay[0] == kind]


def label(lay):
    kind, R, A = lay
    return {"offset": f"offset R={R:g}", "step": f"step R={R:g}", "zerovar": f"zero variance, bias {R:g}", "constch": "constant per channel",
            "outlier": "outlier", "corner": f"first position R={R:g}", "purestep": "step without noise", "control": "control"}[kind]


def bf(t):
    return t.to(torch.bfloat16).to(torch.float32)


# ------------------------------------------------------------------------------------------------ float64 reference + metric
def gn_ref(v, gamma, beta, eps=GN_EPS):
    """v (B, C, ...) -> float64 dict of (B, C) tensors: mean m, biased variance var, s = sqrt(var + eps), a = gamma / s,
    b = beta - m a, and gamma, beta broadcast.  Nothing is rounded to fp32."""
    B, C = v.shape[0], v.shape[1]
    per = C // GROUPS
    g = v.double().reshape(B, GROUPS, -1)
    m = g.mean(dim=2)
    var = ((g - m.unsqueeze(2)) ** 2).mean(dim=2)  # two-pass
    m, var = m.repeat_interleave(per, dim=1), var.repeat_interleave(per, dim=1)
    s = torch.sqrt(var + eps)
    ga, be = gamma.double().view(1, C).expand(B, C), beta.double().view(1, C).expand(B, C)
    a = ga / s
    return {"m": m, "var": var, "s": s, "a": a, "b": be - m * a, "gamma": ga, "beta": be}


def gn_apply_f64(v, ref, relu=False):
    sh = (v.shape[0], v.shape[1]) + (1,) * (v.dim() - 2)
    y = v.double() * ref["a"].view(sh) + ref["b"].view(sh)
    return F.relu(y) if relu else y


def bound(ref, mode):
    """Per (segment, channel) bound of the displacement (module docstring)."""
    return TOL_MODE[mode] + 8 * U32 * ((ref["a"] * ref["m"]).abs() + ref["a"].abs() * 4 * ref["s"] + ref["beta"].abs())


def displacement(coef, ref):
    """coef (B, C, 2): the kernel's (a, b) -> (B, C) displacement."""
    da, db = coef[..., 0].double().cpu() - ref["a"], coef[..., 1].double().cpu() - ref["b"]
    lo, hi = ref["m"] - 4 * ref["s"], ref["m"] + 4 * ref["s"]
    return torch.maximum((da * lo + db).abs(), (da * hi + db).abs())


def element_bound(v, ref, mode):
    """Per-element bound of |a x + b - (a* x + b*)| for every element of v (B, C, ...): the channel's bound, scaled up for the
    elements further than 4 s* from the mean (the displacement is affine in x)."""
    sh = (v.shape[0], v.shape[1]) + (1,) * (v.dim() - 2)
    far = (v.double() - ref["m"].view(sh)).abs() / (4 * ref["s"].view(sh))
    return bound(ref, mode).view(sh) * far.clamp_min(1.0)


def group_worst(disp, bnd):
    """(B, C) displacement and bound -> per group: (worst disp / bound, the disp and the bound of that channel)."""
    ratio = disp / bnd
    out = []
    for g in range(GROUPS):
        sl = ratio[:, 8 * g:8 * g + 8].reshape(-1)
        k = int(sl.argmax())
        out.append((float(sl[k]), float(disp[:, 8 * g:8 * g + 8].reshape(-1)[k]), float(bnd[:, 8 * g:8 * g + 8].reshape(-1)[k])))
    return out


def report(rows):
    """rows: [(kernel, level or shape, group label, disp, bound)] -> table text, the worst row per (kernel, group label)."""
    worst = {}
    for k, where, lab, d, b in rows:
        key = (k, lab)
        if key not in worst or d / b > worst[key][1] / worst[key][2]:
            worst[key] = (where, d, b)
    lines = [f"{'kernel':<34} {'group':<28} {'worst disp':>11} {'bound':>11} {'disp/bound':>10}  at"]
    for (k, lab), (where, d, b) in worst.items():
        lines.append(f"{k:<34} {lab:<28} {d:11.3e} {b:11.3e} {d / b:10.3f}  {where}")
    return "\n".join(lines)


def check_coef(coef, ref, mode, layout, kernel, where, rows=None):
    """Displacement of a coefficient table against its bound, group by group -> list of failure strings (and table rows)."""
    disp, bnd = displacement(coef, ref), bound(ref, mode)
    assert bool(torch.isfinite(coef).all()), f"{kernel} {where}: non-finite coefficients"
    bad = []
    for g, (ratio, d, b) in enumerate(group_worst(disp, bnd)):
        lab = label(layout[g])
        if rows is not None:
            rows.append((kernel, where, lab, d, b))
        if not ratio <= 1.0:
            bad.append(f"{kernel} {where} group {g} ({label(layout[g])}): displacement {d:.3e} > bound {b:.3e}")
    return bad


# ------------------------------------------------------------------------------------------------ crafted inputs
def level_shapes(H, W, n=5):
    h, w = H // 8, W // 8
    out = []
    for _ in range(n):
        out.append((h, w))
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return out


def outlier_pos(h, w):
    return h // 3, w // 3


def crafted_pyramid(B, H, W, seed, cin=256, outlier_at=None):
    """Channel 0 = 1, channel 1 = -1 on the left half of every map and +1 on the right half, channel 2 = bf16 randn with ONE position
    of every map set to 2^12 (read by the outlier group only), channels 3.. = bf16 randn."""
    g = torch.Generator().manual_seed(seed)
    feats = []
    for h, w in level_shapes(H, W):
        x = bf(torch.randn(B, cin, h, w, generator=g))
        x[:, 0] = 1.0
        x[:, 1] = -1.0
        x[:, 1, :, w // 2:] = 1.0
        oy, ox = outlier_pos(h, w) if outlier_at is None else outlier_at
        x[:, 2, oy, ox] = OUTLIER
        feats.append(x)
    return feats


def crafted_layer(seed, layout=LAYOUT, cin=256, const_ch=0, step_ch=1, outlier_ch=2, dense=None, dense_ms=1.0, step_dc=0.0):
    """One cin -> 256 3x3 conv whose output group g has the distribution layout[g] given an input whose channel const_ch is 1,
    whose channel step_ch is step_dc + (-1 left / +1 right), and whose `dense` channels (default: all others) are noise with a summed
    mean square of dense_ms per channel: dense random weights scaled to unit output sigma, the constant and the step read through the
    centre tap only (no border effect), D and A powers of two.  Weights are bf16-exact.  -> (weight, bias)."""
    g = torch.Generator().manual_seed(seed)
    special = {const_ch, step_ch, outlier_ch}
    dense = [c for c in range(cin) if c not in special] if dense is None else list(dense)
    w = torch.zeros(256, cin, 3, 3)
    std = 1.0 / math.sqrt(9 * len(dense) * dense_ms)
    w[:, dense] = torch.randn(256, len(dense), 3, 3, generator=g) * std
    bias = 0.1 * torch.randn(256, generator=g)
    for gi, (kind, R, A) in enumerate(layout):
        ch = slice(8 * gi, 8 * gi + 8)
        if kind in ("zerovar", "constch", "purestep"):
            w[ch] = 0.0
        if kind == "zerovar":
            bias[ch] = R
        elif kind == "constch":
            bias[ch] = torch.tensor(CONSTCH_BIASES)
        elif kind == "purestep":
            bias[ch] = 0.0
            w[ch, step_ch, 1, 1] = A
            w[ch, const_ch, 1, 1] = -A * step_dc
        elif kind in ("offset", "step"):
            w[ch, const_ch, 1, 1] = R - A * step_dc
            w[ch, step_ch, 1, 1] = A
        elif kind == "corner":  # R sigma on all eight channels where the outlier channel holds 2^12, through the centre tap
            w[ch, outlier_ch, 1, 1] = R / OUTLIER
        elif kind == "outlier" and outlier_ch is not None:
            w[ch, outlier_ch] = torch.randn(8, 3, 3, generator=g) * std
    return bf(w), bias


def gn_params(seed, layout=LAYOUT, unit_groups=()):
    """gamma = 1 + 0.1 randn, beta = 0.1 randn; gamma = beta = 1 on `unit_groups` (their normalised output feeds the next crafted
    layer: relu(beta) = 1 for a zero-variance group)."""
    g = torch.Generator().manual_seed(seed)
    gamma, beta = 1.0 + 0.1 * torch.randn(256, generator=g), 0.1 * torch.randn(256, generator=g)
    for gi in unit_groups:
        gamma[8 * gi:8 * gi + 8] = 1.0
        beta[8 * gi:8 * gi + 8] = 1.0
    return gamma, beta


def conv_f64(x, w, bias):
    """3x3 pad-1 conv + bias in float64 on the operands as given."""
    return F.conv2d(x.double(), w.double(), bias.double(), padding=1)


def measured(v, layout, bias):
    """Float64 epilogue values v (B, 256, h, w) -> per group: R = |group mean - bias of the group's first channel| / sigma_noise (the
    worst image), the share of the variance that lies between the left and the right half, the variance (the smallest image's).
    sigma_noise is the within-half standard deviation about each channel's own half mean ... for the groups with noise."""
    B, _, h, w = v.shape
    out = []
    for gi in range(GROUPS):
        x = v[:, 8 * gi:8 * gi + 8].double()
        m = x.mean(dim=(1, 2, 3))
        var = ((x - m.view(B, 1, 1, 1)) ** 2).mean(dim=(1, 2, 3))
        left, right = x[..., :w // 2], x[..., w // 2:]
        nl, nr = left[0].numel(), right[0].numel()
        ml = left.mean(dim=(1, 2, 3)) if nl else m
        mr = right.mean(dim=(1, 2, 3))
        between = (nl * (ml - m) ** 2 + nr * (mr - m) ** 2) / (nl + nr)
        noise = torch.sqrt((var - between).clamp_min(0.0))
        R = ((m - float(bias[8 * gi])).abs() / noise.clamp_min(1e-30)).max()
        out.append({"R": float(R), "step_share": float((between / var.clamp_min(1e-300)).min()), "var": float(var.min()),
                    "var_max": float(var.max())})
    return out


def direct_groups(B, H, W, seed, layout=LAYOUT):
    """The same distributions written directly into a (B, 256, H, W) tensor (the stand-alone GroupNorm's operand), sigma = 1."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 256, H, W, generator=g)
    step = torch.where(torch.arange(W) >= W // 2, 1.0, -1.0).view(1, 1, 1, W)
    for gi, (kind, R, A) in enumerate(layout):
        ch = slice(8 * gi, 8 * gi + 8)
        if kind in ("offset", "step"):
            x[:, ch] += R + A * step
        elif kind == "zerovar":
            x[:, ch] = R
        elif kind == "constch":
            x[:, ch] = torch.tensor(CONSTCH_BIASES).view(1, 8, 1, 1)
        elif kind == "purestep":
            x[:, ch] = (A * step).expand(B, 8, H, W)
        elif kind == "outlier":
            oy, ox = outlier_pos(H, W)
            x[:, ch, oy, ox] = OUTLIER * torch.sign(x[:, ch, oy, ox])
    return x
