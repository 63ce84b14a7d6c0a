"""GroupNorm statistics of every kernel that computes them, pinned to float64 on groups that are off their pivot, stepped between
tiles, constant, or dominated by one outlier (tests/gn_stats_ref.py builds the inputs and states the bound).

  1. stand-alone GroupNorm (gn_stats_kernel -> gn_finalize_kernel -> gn_apply_kernel), f32 and bf16, from one position to nine
     row chunks with a ragged last one;
  2. conv_igemm's epilogue partials (gn_tile_reduce) in bf16, f32 and f32s on a 128 x 160 pyramid;
  3. conv_hpipe<false> and <true> on one 800 x 1344 pyramid (94 blocks: the smallest launch that is still on conv_hpipe);
  4. conv_deform's epilogue partials (a two-layer tower whose deformable last layer has zero offsets);
  5. the finalizer's tail loop: a P3 segment of more than 256 conv_hpipe partials;
  6. the support tower's 49-row segments, bf16 and f32;
  7. conv_hpipe's pivot sample (the first position of a patch) on a map whose first position is an outlier of its group.
Each conv case checks the (a, b) table of every (image, level, channel) with the displacement metric and the stored pre-GroupNorm
output to one bf16 ulp (per group: the ulp floor of one group is not raised by another group's magnitude); the fp32 modes, which
keep no table, compare the layer's output after GroupNorm + ReLU element by element with the float64 layer -- there the fp32 conv's
own accumulation error (an offset group carries its D through all K additions: 9e-3 allowed at R = 1024 against 7e-4 for the
GroupNorm) limits what a large-R group can show; the fp32 statistics at large R are pinned by the support-tower f32 case, whose
coefficient table is held to the 1e-4 metric.  Each case asserts the
kernels and conv routes that ran.  Each prints its table of worst displacement and bound per kernel and group."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import gn_stats_ref as G
from bf16_ulps import assert_ulps, bf16_rne, ulps

pytestmark = pytest.mark.gpu

P = "proposal_generator.fcos_head"
TOWERS = ((0, "cls_tower"), (1, "bbox_tower"))
LAYOUT1 = [lay if lay[0] != "outlier" else ("control", 0.0, 0.0) for lay in G.LAYOUT]  # a second crafted layer has no outlier channel
HP_T, HP_F, IGK, DFK = "conv_hpipe_kernel<true>", "conv_hpipe_kernel<false>", "conv_igemm_kernel", "conv_deform_kernel"
TAPS, LOGITS = "gn_taps_kernel+tap_gather_kernel", "gn_logits_kernel"
HP, IG64 = "hpipe 256x256", "igemm 64x64 nbuf3"


def _cfg(deformable=False, num_convs=4):
    from sylph_amd.config import get_default_cfg
    cfg = get_default_cfg()
    cg = cfg.MODEL.META_LEARN.CODE_GENERATOR
    cfg.MODEL.META_LEARN.EPISODIC_LEARNING = True
    cg.CONV_L2_NORM = True
    cg.TOWER_LAYERS = [["GN", "ReLU"], ["GN", "ReLU"]]
    cg.CLS_LAYER = ["", "", 1]
    cg.BIAS_LAYER = ["", "", 1]
    cfg.MODEL.FCOS.USE_DEFORMABLE = deformable
    cfg.MODEL.FCOS.NUM_CLS_CONVS = num_convs
    cfg.MODEL.FCOS.NUM_BOX_CONVS = num_convs
    return cfg


def _routing_overrides():
    return sorted(k for k in os.environ if k.startswith(("SYLPH_CONV_", "SYLPH_SPLIT_", "SYLPH_FUSE_")))


def _assert_forms(eng, kernels, routes, what):
    """As tests/test_bf16_pinned_gpu.py: the kernels that ran and the conv routes that were built are the ones the case names (not
    under the routing overrides of the forced-variant reruns)."""
    got_k, got_r = list(eng.profile_read()["kernels"]), eng.conv_routes()
    print(f"{what}: kernels {got_k}, conv routes {got_r}")
    if _routing_overrides():
        return
    assert got_k == kernels and got_r == routes, f"{what}: expected kernels {kernels} / routes {routes}, ran {got_k} / {got_r}"


def _finish(rows, bad, what):
    print(f"---- GroupNorm statistics: {what}\n{G.report(rows)}")
    assert not bad, f"{len(bad)} (segment, group) over the bound:\n" + "\n".join(bad[:40])


def _check_y(y, v, layout, what):
    """Stored bf16 pre-GroupNorm output against the float64 conv rounded once: <= 1 % of elements differ, each group within 1 ulp
    (floor 1e-3 of THAT group's maximum)."""
    want = bf16_rne(v)
    assert_ulps(y, want, what)
    for g in range(G.GROUPS):
        _, worst = ulps(y[:, 8 * g:8 * g + 8], want[:, 8 * g:8 * g + 8])
        assert worst <= 1.0, f"{what} group {g} ({G.label(layout[g])}): worst {worst:.2f} bf16 ulp"


def _head_engine(dtype, sd, feats, hw, cfg):
    from sylph_amd import synthetic as Wt
    from sylph_amd.engine import Engine
    eng = Engine(cfg, dtype=dtype)
    eng.load_state_dict(sd)
    eng.set_debug_taps(True)
    eng.profile_enable(True)
    eng.import_pyramid(feats, hw)
    codes = Wt.synthetic_codes(5, seed=4, scale=3.0)
    eng.head(codes["cls_conv"], codes["cls_bias"])
    return eng


def _set_layer(sd, name, i, w, bias, gamma, beta, deform=False):
    k = f"{P}.{name}.{3 * i}"
    if deform:
        sd[f"{k}.conv.weight"], sd[f"{k}.conv.bias"] = w, bias
        sd[f"{k}.offset.weight"].zero_()
        sd[f"{k}.offset.bias"].zero_()
        sd[f"{k}.offset.bias"][18:] = 40.0  # sigmoid(40) == 1.0f: the deformable conv is the plain one
    else:
        sd[f"{k}.weight"], sd[f"{k}.bias"] = w, bias
    sd[f"{P}.{name}.{3 * i + 1}.weight"], sd[f"{P}.{name}.{3 * i + 1}.bias"] = gamma, beta


# ------------------------------------------------------------------------------------------------ 1. stand-alone GroupNorm
GN_SHAPES = [(1, 1, 1), (2, 7, 7), (1, 33, 41), (1, 40, 52)]
assert (40 * 52 + 255) // 256 == 9 and 40 * 52 % 256 != 0  # GN_ROWS_PER_CHUNK = 256: nine chunks, the last one ragged


@pytest.mark.parametrize("shape", GN_SHAPES, ids=["x".join(map(str, s)) for s in GN_SHAPES])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_standalone_group_norm(dtype, shape):
    """Engine.group_norm on the crafted distributions written directly into x; 40 x 52 = 2080 rows are nine chunks of 256 rows, the
    last one of 32.  Against float64 GroupNorm of the stored operand, element by element, within the metric's bound (+ one bf16 ulp
    of the output element where the output is stored in bf16); the zero-variance groups come out finite."""
    from sylph_amd.engine import Engine
    B, H, W = shape
    x = G.direct_groups(B, H, W, seed=100 + H)
    if dtype == "bf16":
        x = G.bf(x)
    gamma, beta = G.gn_params(7)
    eng = Engine(_cfg(), dtype=dtype)
    eng.profile_enable(True)
    y = eng.group_norm(x, gamma, beta, relu=False).cpu()
    # a negative assertion only: the profile records conv launches, and none may run here.  sylph_group_norm has one code path
    # (gn_stats_kernel -> gn_finalize_kernel -> gn_apply_kernel); nothing positive pins it.
    _assert_forms(eng, [], [], f"group_norm {dtype} {shape}")
    assert bool(torch.isfinite(y).all()), "non-finite GroupNorm output"
    ref = G.gn_ref(x, gamma, beta)
    want = G.gn_apply_f64(x, ref)
    tol = G.element_bound(x, ref, dtype)
    if dtype == "bf16":
        mag = torch.maximum(want.abs(), y.double().abs()).clamp_min(2.0 ** -126)
        tol = tol + torch.exp2(torch.floor(torch.log2(mag)) - 7)
    err = (y.double() - want).abs()
    rows, bad = [], []
    for g in range(G.GROUPS):
        e, t = err[:, 8 * g:8 * g + 8].reshape(-1), tol[:, 8 * g:8 * g + 8].reshape(-1)
        k = int((e / t).argmax())
        rows.append((f"gn_stats_kernel {dtype}", "x".join(map(str, shape)), G.label(G.LAYOUT[g]), float(e[k]), float(t[k])))
        if not float(e[k]) <= float(t[k]):
            bad.append(f"group {g} ({G.label(G.LAYOUT[g])}): |y - y*| {float(e[k]):.3e} > {float(t[k]):.3e}")
    _finish(rows, bad, f"stand-alone GroupNorm {dtype} {shape} (element error instead of displacement)")


# ------------------------------------------------------------------------------------------------ 2. conv_igemm partials
def _conv_error(x, w, dtype):
    """Per-element allowance for the fp32-mode conv itself against the float64 conv.  fp32 accumulation of K = 9 Cin products: every
    addition rounds by at most half an ulp of the partial sum, uniformly, i.e. with a standard deviation of 2^-23 |partial| / sqrt(12)
    <= 2^-23 sum |w x| / sqrt(12); K independent roundings, six standard deviations (the worst of ~10^5 elements):
    6 / sqrt(12) * 2 = 3.5 sqrt(K) 2^-24 sum |w x|.  (An offset group carries its D = 1024 through all K additions: 3e-3 at
    D = 1024 is what fp32 accumulation costs there, whatever the GroupNorm does.)  f32s splits each operand into hi + lo with lo
    rounded to bf16, 2^-17 relative, and drops the lo x lo term, 2^-18: 1.25 * 2^-16 per product, independent over the products,
    six standard deviations of their sum -- and nothing where both operands are exact in bf16 (lo = 0), as the crafted ones are."""
    sabs = F.conv2d(x.double().abs(), w.double().abs(), None, padding=1)
    err = 6.0 / math.sqrt(12.0) * 2.0 * math.sqrt(9 * x.shape[1]) * G.U32 * sabs
    if dtype == "f32s" and not (torch.equal(G.bf(x), x) and torch.equal(G.bf(w), w)):
        err = err + 6 * 1.25 * 2.0 ** -16 * torch.sqrt(F.conv2d(x.double() ** 2, w.double() ** 2, None, padding=1))
    return err


IGEMM_FORMS = {
    "bf16": ([IGK, TAPS, LOGITS], [IG64] * 2),
    "f32": ([IGK], ["igemm 64x64"] * 8 + ["igemm 128x32"]),
    "f32s": ([IGK], ["igemm 64x64"] * 8 + ["igemm 128x32"]),
}


@pytest.mark.parametrize("dtype", ["bf16", "f32", "f32s"])
def test_conv_igemm_partials(dtype):
    """The crafted layer as layer 0 of both towers, two 128 x 160 pyramids (levels 16 x 20 ... 1 x 2: several 64-row tiles at P3,
    ragged single tiles above).  bf16: one-layer towers, because only a tower's last layer keeps its coefficient table and its
    pre-GroupNorm output on this route (the others are normalised in place); f32 / f32s: the usual four layers, layer 0's output
    after GroupNorm + ReLU."""
    from sylph_amd import synthetic as Wt
    Hh, Ww, B = 128, 160, 2
    feats = G.crafted_pyramid(B, Hh, Ww, seed=31)
    nconv = 1 if dtype == "bf16" else 4
    sd = Wt.head_state_dict(seed=1, num_classes=60, num_convs=nconv)
    layers = {}
    for t, name in TOWERS:
        layers[name] = G.crafted_layer(40 + t) + G.gn_params(50 + t)
        _set_layer(sd, name, 0, *layers[name])
    eng = _head_engine(dtype, sd, feats, (Hh, Ww), _cfg(num_convs=nconv))
    _assert_forms(eng, *IGEMM_FORMS[dtype], f"conv_igemm partials {dtype}")
    rows, bad = [], []
    for t, name in TOWERS:
        w, bias, gamma, beta = layers[name]
        ys, cfs = eng.export_tower(t, 0, with_coef=dtype == "bf16")
        for l, x in enumerate(feats):
            v = G.conv_f64(x, w, bias)
            ref = G.gn_ref(v, gamma, beta)
            where = f"{name} level {l}"
            if dtype == "bf16":
                bad += G.check_coef(cfs[l].cpu(), ref, dtype, G.LAYOUT, f"conv_igemm {dtype}", where, rows)
                _check_y(ys[l].cpu(), v, G.LAYOUT, f"conv_igemm bf16 {where} stored output")
                continue
            got = ys[l].cpu().double()
            assert bool(torch.isfinite(got).all()), where
            want = G.gn_apply_f64(v, ref, relu=True)
            tol = G.element_bound(v, ref, dtype) + ref["a"].abs().view(B, 256, 1, 1) * _conv_error(x, w, dtype)
            err = (got - want).abs()
            for g in range(G.GROUPS):
                e, tl = err[:, 8 * g:8 * g + 8].reshape(-1), tol[:, 8 * g:8 * g + 8].reshape(-1)
                k = int((e / tl).argmax())
                rows.append((f"conv_igemm {dtype}", where, G.label(G.LAYOUT[g]), float(e[k]), float(tl[k])))
                if not float(e[k]) <= float(tl[k]):
                    bad.append(f"{where} group {g} ({G.label(G.LAYOUT[g])}): |y - y*| {float(e[k]):.3e} > {float(tl[k]):.3e}")
    _finish(rows, bad, f"conv_igemm partials {dtype}" + ("" if dtype == "bf16" else " (element error of the layer output)"))


# ------------------------------------------------------------------------------------------------ 3. + 4. two crafted layers
def _second_layer(seed, feats, w0, b0, ga0, be0):
    """The crafted layer that reads the first one's output: its constant channel is the first layer's zero-variance group
    (relu(beta) = 1), its step channel the noise-free step group (relu(1 -+ 1): 1 + step), its dense channels the control groups,
    whose mean square comes from the float64 first layer."""
    dense = [c for g in G.groups_of(G.LAYOUT, "control") for c in range(8 * g, 8 * g + 8)]
    ssq, n = 0.0, 0
    for x in feats:
        v = G.conv_f64(x, w0, b0)
        out = G.gn_apply_f64(v, G.gn_ref(v, ga0, be0), relu=True)[:, dense]
        ssq, n = ssq + float((out ** 2).sum()), n + out.numel()
    return G.crafted_layer(seed, layout=LAYOUT1, const_ch=8 * G.G_ZERO, step_ch=8 * G.G_PURESTEP, outlier_ch=None, dense=dense,
                           dense_ms=ssq / n, step_dc=1.0)


def _check_measured(v, layout, bias, what):
    """The second layer's groups are as far off their pivot as their names say.  Its inputs come from the HIP graph and have a
    non-zero mean (ReLU outputs), which gives every output channel a constant of its own, ~0.6 sigma: a group's spread differs from
    1 by more than the first layer's, so R is held to 30 % + 1."""
    got = G.measured(v, layout, bias)
    for g, (kind, R, A) in enumerate(layout):
        if kind in ("offset", "step"):
            print(f"{what} group {g} ({G.label(layout[g])}): measured R {got[g]['R']:.2f}, step share {got[g]['step_share']:.3f}")
            assert abs(got[g]["R"] - R) <= 0.3 * R + 1.0, (what, g, got[g])
            assert kind != "step" or got[g]["step_share"] > 0.9, (what, g, got[g])


def _two_layer_case(hw, B, deformable, kernels, routes, names):
    from oracle import bf16 as OB16
    from sylph_amd import synthetic as Wt
    feats = G.crafted_pyramid(B, hw[0], hw[1], seed=61)
    nconv = 2 if deformable else 4
    sd = Wt.head_state_dict(seed=1, num_classes=60, num_convs=nconv, deformable=deformable)
    layers = {}
    for t, name in TOWERS:
        l0 = G.crafted_layer(70 + t) + G.gn_params(80 + t, unit_groups=(G.G_ZERO, G.G_PURESTEP))
        l1 = _second_layer(90 + t, feats, *l0) + G.gn_params(95 + t)
        layers[name] = (l0, l1)
        _set_layer(sd, name, 0, *l0)
        _set_layer(sd, name, 1, *l1, deform=deformable)
    eng = _head_engine("bf16", sd, feats, hw, _cfg(deformable, nconv))
    _assert_forms(eng, kernels, routes, names[1])
    rows, bad = [], []
    for t, name in TOWERS:
        (w0, b0, ga0, be0), (w1, b1, ga1, be1) = layers[name]
        ys0, cfs0 = eng.export_tower(t, 0, with_coef=not deformable)
        ys1, cfs1 = eng.export_tower(t, 1)
        for l, x in enumerate(feats):
            where = f"{name} level {l}"
            if deformable:  # layer n-2 of a deformable tower is normalised in place: the tap is the second layer's operand
                x1 = ys0[l].cpu()
            else:
                v0 = G.conv_f64(x, w0, b0)
                bad += G.check_coef(cfs0[l].cpu(), G.gn_ref(v0, ga0, be0), "bf16", G.LAYOUT, names[0], where, rows)
                _check_y(ys0[l].cpu(), v0, G.LAYOUT, f"{names[0]} {where} stored output")
                x1 = OB16.gn_apply(ys0[l].cpu(), cfs0[l].cpu())  # the second layer's operand from the HIP graph's own values
            v1 = G.conv_f64(x1, w1, b1)
            if l == 0:
                _check_measured(v1, LAYOUT1, b1, f"{names[1]} {where}")
            bad += G.check_coef(cfs1[l].cpu(), G.gn_ref(v1, ga1, be1), "bf16", LAYOUT1, names[1], where, rows)
            _check_y(ys1[l].cpu(), v1, LAYOUT1, f"{names[1]} {where} stored output")
    _finish(rows, bad, " + ".join(n for n in names if n))


def test_conv_hpipe_plain_and_groupnorm_in():
    """One 800 x 1344 pyramid: 94 blocks per tower layer, the smallest launch on conv_hpipe.  Layer 0 (conv_hpipe<false>) is the
    crafted layer, layer 1 (conv_hpipe<true>: the previous GroupNorm + ReLU applied to its input halo) a crafted layer on layer 0's
    output, its reference built from the HIP graph's own layer-0 output and coefficients."""
    _two_layer_case((800, 1344), 1, False, [HP_F, HP_T, TAPS, LOGITS], [HP] * 8, ("conv_hpipe<false>", "conv_hpipe<true>"))


def test_conv_deform_partials():
    """MODEL.FCOS.USE_DEFORMABLE, two-layer towers on two 128 x 160 pyramids: the crafted second layer is the deformable one, with
    zero offsets and a saturated mask (conv_deform_kernel's epilogue, gn_tile_reduce)."""
    _two_layer_case((128, 160), 2, True, [IGK, DFK, TAPS, LOGITS], [IG64, "igemm 128x32"] * 2, ("", "conv_deform"))


# ------------------------------------------------------------------------------------------------ 5. finalizer tail
def test_finalizer_tail_beyond_256_partials():
    """One 1480 x 1480 image: P3 is 185 x 185 = 34 225 positions, more than 256 conv_hpipe patches of 128 positions, so the P3 segment
    runs the plain loop of gn_finalize_partials_kernel behind its 8 prefetched links per chain.  Step groups (tiles 16 sigma apart): a
    dropped or repeated tile shifts the mean by whole sigmas.  The crafted layer reads 64 input channels (float64 conv time)."""
    from sylph_amd import synthetic as Wt
    hw = (1480, 1480)
    h, w_ = G.level_shapes(*hw)[0]
    assert h * w_ > 256 * 128, "ntiles = ceil(positions / 128) > 256 needs more than 32 768 positions"
    feats = G.crafted_pyramid(1, hw[0], hw[1], seed=111)
    sd = Wt.head_state_dict(seed=1, num_classes=60)
    layers = {}
    for t, name in TOWERS:
        layers[name] = G.crafted_layer(120 + t, layout=G.STEP_ONLY_LAYOUT, dense=range(3, 64)) + G.gn_params(130 + t)
        _set_layer(sd, name, 0, *layers[name])
    eng = _head_engine("bf16", sd, feats, hw, _cfg())
    _assert_forms(eng, [HP_F, HP_T, TAPS, LOGITS], [HP] * 8, "finalizer tail")
    rows, bad = [], []
    for t, name in TOWERS:
        w, bias, gamma, beta = layers[name]
        assert float(w[:, 64:].abs().max()) == 0.0
        ys, cfs = eng.export_tower(t, 0)
        for l, x in enumerate(feats):
            v = G.conv_f64(x[:, :64], w[:, :64], bias)
            bad += G.check_coef(cfs[l].cpu(), G.gn_ref(v, gamma, beta), "bf16", G.STEP_ONLY_LAYOUT, "gn_finalize_partials (tail)",
                                f"{name} level {l}", rows)
            _check_y(ys[l].cpu(), v, G.STEP_ONLY_LAYOUT, f"finalizer tail {name} level {l} stored output")
    _finish(rows, bad, "finalizer tail, 268 or more partials at P3")


def test_conv_hpipe_pivot_when_first_position_is_an_outlier():
    """conv_hpipe moves a (patch, group)'s pivot to the mean of the patch's first position when that lies far from the conv bias.
    Here position (0, 0) of every map -- the first position of its first patch -- carries 64 or 1024 sigma on all eight channels of a
    group whose other positions sit on the bias (and, third group, 2^12 through dense weights: eight different values): the one input
    on which the sampled pivot is worse than the bias.  It stays harmless because the sampled value is part of the patch's own spread."""
    from sylph_amd import synthetic as Wt
    hw = (800, 1344)
    feats = G.crafted_pyramid(1, hw[0], hw[1], seed=161, outlier_at=(0, 0))
    sd = Wt.head_state_dict(seed=1, num_classes=60)
    layers = {}
    for t, name in TOWERS:
        layers[name] = G.crafted_layer(170 + t, layout=G.CORNER_LAYOUT) + G.gn_params(180 + t)
        _set_layer(sd, name, 0, *layers[name])
    eng = _head_engine("bf16", sd, feats, hw, _cfg())
    _assert_forms(eng, [HP_F, HP_T, TAPS, LOGITS], [HP] * 8, "first-position outlier")
    rows, bad = [], []
    for t, name in TOWERS:
        w, bias, gamma, beta = layers[name]
        ys, cfs = eng.export_tower(t, 0)
        for l, x in enumerate(feats):
            v = G.conv_f64(x, w, bias)
            for g, (kind, R, A) in enumerate(G.CORNER_LAYOUT):
                if kind == "corner":  # the crafted value is there, on all eight channels, and nowhere else
                    assert float((v[0, 8 * g:8 * g + 8, 0, 0] - R).abs().max()) < 6.0 and float(v[0, 8 * g:8 * g + 8, 2:, 2:].abs().max()) < 8.0
            bad += G.check_coef(cfs[l].cpu(), G.gn_ref(v, gamma, beta), "bf16", G.CORNER_LAYOUT, "conv_hpipe<false> (pivot sample)",
                                f"{name} level {l}", rows)
            _check_y(ys[l].cpu(), v, G.CORNER_LAYOUT, f"first-position outlier {name} level {l} stored output")
    _finish(rows, bad, "conv_hpipe, first position of a patch an outlier")


# ------------------------------------------------------------------------------------------------ 6. support tower
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_support_tower_49_row_segments(dtype):
    """codegen_classes, 2 classes x 2 shots on crafted 128 x 160 pyramids with boxes inside the image (ROIAlign of the constant
    channel is 1); support_set_shared_tower.0 is the crafted layer with its offset, zero-variance and control groups."""
    from oracle import bf16 as OB16
    from oracle.codegen import CG_PREFIX
    from sylph_amd import synthetic as Wt
    from sylph_amd.engine import Engine
    hw, S = (128, 160), 4
    feats = G.crafted_pyramid(S, hw[0], hw[1], seed=141)
    boxes = torch.tensor([[16.0, 12.0, 100.0, 90.0], [40.5, 30.25, 120.0, 110.0], [8.0, 8.0, 150.0, 120.0], [60.0, 20.0, 130.0, 70.0]])
    roi_cpu = OB16.roi_pool(feats, boxes)
    dense = list(range(3, 256))
    sd = Wt.codegen_state_dict(seed=2)
    p = f"{CG_PREFIX}.support_set_shared_tower"
    w, bias = G.crafted_layer(150, layout=G.SUPPORT_LAYOUT, dense=dense, dense_ms=float((roi_cpu[:, dense].double() ** 2).mean()))
    gamma, beta = G.gn_params(151)
    sd[f"{p}.0.weight"], sd[f"{p}.0.bias"], sd[f"{p}.1.weight"], sd[f"{p}.1.bias"] = w, bias, gamma, beta
    eng = Engine(_cfg(), dtype=dtype)
    eng.load_state_dict(sd)
    eng.set_debug_taps(True)
    eng.profile_enable(True)
    eng.import_pyramid(feats, hw)
    eng.codegen_classes(boxes, 2)
    tower = IG64 if dtype == "bf16" else "igemm 64x64"
    _assert_forms(eng, [IGK], [tower] * 3 + ["igemm 128x32"], f"support tower {dtype}")
    x = eng.export_support("roi").cpu()
    assert float((x[:, 0] - 1.0).abs().max()) <= 2.0 ** -8, "ROIAlign of the constant channel"
    v = G.conv_f64(x, w, bias)
    got = G.measured(v, G.SUPPORT_LAYOUT, bias)
    for g, (kind, R, A) in enumerate(G.SUPPORT_LAYOUT):
        if kind == "offset":
            print(f"support tower group {g}: measured R {got[g]['R']:.2f}")
            assert got[g]["R"] >= 0.8 * R, (g, got[g])  # (the ROI maps of large boxes are smoother: the worst image is further off)
    rows = []
    bad = G.check_coef(eng.export_support("gn_coef", 0).cpu(), G.gn_ref(v, gamma, beta), dtype, G.SUPPORT_LAYOUT,
                       f"support tower (conv_igemm) {dtype}", "2 x 2 shots", rows)
    y = eng.export_support("gn_y", 0).cpu()
    if dtype == "bf16":
        _check_y(y, v, G.SUPPORT_LAYOUT, "support tower stored output")
    else:
        assert bool(((y.double() - v).abs() <= _conv_error(x, w, dtype) + 4 * G.U32 * v.abs()).all()), "support tower fp32 conv output"
    _finish(rows, bad, f"support tower {dtype}")
