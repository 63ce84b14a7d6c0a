"""Meta-training of the code generator on the GPU (csrc/codegen_train.hip through Engine.codegen_train_forward / codegen_train_backward,
Engine.roi_rows, Engine.set_code_generator and sylph_amd.metatrain.train_code_generator).

Yardsticks: tests/codegen_train_ref.py, pinned to the reference's own CodeGenerator by tests/test_codegen_train_cpu.py.  Every exported
stage is recomputed in float64 from the kernel's own exported inputs of that stage -- conv weights and d y rounded to bf16 where the kernels
round them, the ReLU mask from the saved activation, mean / rstd as saved -- and held to
    |err| <= (fp32 roundings of the chain + summation length) * 2^-24 * (the same expression over absolute values):
the worst case of an fp32 chain, no measured constant.  x_{i+1} is stored in bf16: its bound adds the half ulp, at most 2^-8 |value|.
Everything else is bit equality between two runs of the library, or a comparison of two errors against float64."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import codegen_train_ref as R
import finetune_ref as FR

pytestmark = pytest.mark.gpu
E = 2.0 ** -24
P = R.P
VARIANTS = [(True, True), (False, True), (False, False)]  # (POST_NORM "GN", CONV_L2_NORM)


def _cfg(depth=2, post_norm=True, l2=True, bias=True):
    from test_hip_parity import _cfg as base
    cfg = base()
    cg = cfg.MODEL.META_LEARN.CODE_GENERATOR
    cg.TOWER_LAYERS = [["GN", "ReLU"]] * depth
    cg.POST_NORM = "GN" if post_norm else ""
    cg.CONV_L2_NORM = bool(l2)
    cg.BIAS_LAYER = ["", "", 1] if bias else []
    return cfg


def _gen_sd(depth, seed=2):
    from sylph_amd import synthetic as W
    return W.codegen_state_dict(seed=seed, tower_layers=depth)


def _engine(depth=2, post_norm=True, l2=True, bias=True, dtype="bf16", extra=None, cfg=None):
    from sylph_amd.engine import Engine
    eng = Engine(cfg if cfg is not None else _cfg(depth, post_norm, l2, bias), dtype=dtype)
    sd = dict(extra or {})
    sd.update(_gen_sd(depth))
    eng.load_state_dict(sd)
    return eng


def _kw(depth, post_norm, l2, bias):
    return dict(tower_layers=depth, has_bias=bias, post_norm=post_norm, conv_l2_norm=l2)


def _bank(n, seed):
    """n synthetic bank rows: bf16 values in [0, 2), as ROI maps of a ReLU pyramid would be"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, 49, 256, generator=g) * 2.0).to(torch.bfloat16)


def _params(eng, sd=None):
    """(flat fp32 vector, layout) of a state dict (default: the engine's own generator)"""
    lay = eng.codegen_params()
    if sd is None:
        return eng.code_generator(), lay
    return torch.cat([sd[k].float().reshape(-1) for k, _, _ in lay]), lay


def _unflat(flat, lay):
    from sylph_amd.engine import Engine
    return {k: flat[o:o + n].reshape(Engine.codegen_param_shape(k, n)) for k, o, n in lay}


def _maps(t):  # (M * 49, 256) or (M, 49, 256) -> (M, 256, 7, 7) float64
    return R.rows_to_maps(t.reshape(-1, 49, 256).double().cpu())


def _rows(t):  # (M, C, 7, 7) -> (M * 49, C)
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _chk(name, got, want, absexpr, count, extra=None):
    got, want, absexpr = got.double().cpu().reshape(-1), want.double().reshape(-1), absexpr.double().reshape(-1)
    bound = count * E * absexpr + (extra.double().reshape(-1) if extra is not None else 0.0)
    err = (got - want).abs()
    worst = int(torch.argmax(err - bound))
    assert bool((err <= bound).all()), f"{name}: |err| {float(err[worst]):.3e} above the bound {float(bound[worst]):.3e} at {worst} (count {count})"
    assert float(want.abs().max()) > 0 or float(got.abs().max()) == 0, name


# the input positions tap k of a padded 3x3 conv reads over the 7 outputs of an axis: k = 0 reads p - 1, k = 2 reads p + 1
_BOX = (slice(0, 6), slice(0, 7), slice(1, 7))


def _gn_stats64(y):  # (M, 256, 7, 7) -> mean, rstd (M, 32)
    g = y.reshape(y.shape[0], 32, -1)
    return g.mean(2), 1.0 / torch.sqrt(g.var(2, unbiased=False) + 1e-5)


def _stage_check(eng, kw, rows, idx, seg_len, seed=5):
    """one forward + backward with the debug export, every stage against float64 from the kernel's own inputs; -> (codes, grad, stages)"""
    L, M, n_seg = kw["tower_layers"], len(idx), len(seg_len)
    flat, lay = _params(eng)
    p = {k: v.double() for k, v in _unflat(flat, lay).items()}
    dev = flat.cuda()
    codes = eng.codegen_train_forward(dev, rows, idx, seg_len)
    g = torch.Generator().manual_seed(seed)
    G = torch.randn(n_seg, 257, generator=g)
    grad, st = eng.codegen_train_backward(G.cuda(), debug=True)
    grads = {k: v.double().cpu() for k, v in _unflat(grad, lay).items()}
    st = {k: v.double().cpu() for k, v in st.items()}
    x = _maps(rows.cpu()[torch.tensor(idx)])
    xs = [x]
    ex = lambda t, C=256: t[:, :, None, None].expand(M, C, 7, 7)
    # ---- forward
    for i in range(L):
        w, b = R.rbf(p[f"{P}.support_set_shared_tower.{3 * i}.weight"]), p[f"{P}.support_set_shared_tower.{3 * i}.bias"]
        ga, be = p[f"{P}.support_set_shared_tower.{3 * i + 1}.weight"], p[f"{P}.support_set_shared_tower.{3 * i + 1}.bias"]
        _chk(f"y{i}", st[f"y{i}"], _rows(F.conv2d(xs[i], w, b, padding=1)), _rows(F.conv2d(xs[i].abs(), w.abs(), b.abs(), padding=1)), 2304 + 2)
        y = _maps(st[f"y{i}"])
        mean, rstd = _gn_stats64(y)
        amean = y.abs().reshape(M, 32, -1).mean(2)
        _chk(f"mean{i}", st[f"stats{i}"][..., 0], mean, amean, 392 + 2)
        _chk(f"rstd{i}", st[f"stats{i}"][..., 1], rstd, rstd, 392 + 8)
        sm, sr = (st[f"stats{i}"][..., j].repeat_interleave(8, dim=1) for j in (0, 1))
        v = F.relu((y - ex(sm)) * ex(sr) * ga.view(1, -1, 1, 1) + be.view(1, -1, 1, 1))
        av = (y.abs() + ex(sm).abs()) * ex(sr) * ga.abs().view(1, -1, 1, 1) + be.abs().view(1, -1, 1, 1)
        _chk(f"x{i + 1}", st[f"x{i + 1}"], _rows(v), _rows(av), 6, extra=_rows(v.abs() + 6 * E * av) * 2.0 ** -8)
        xs.append(_maps(st[f"x{i + 1}"]))
        assert torch.equal(R.rbf(xs[-1]), xs[-1]), "x is stored in bf16"
    xL = xs[-1]
    xsum = torch.stack([xL[:, :, _BOX[t // 3], _BOX[t % 3]].sum((2, 3)) for t in range(9)], 1).reshape(M, 2304)  # [s][tap][ci]
    _chk("xsum", st["xsum"], xsum, xsum.abs(), 49)
    xs_k = st["xsum"]
    wc = R.rbf(p[f"{P}.support_set_cls_conv.0.weight"]).permute(0, 2, 3, 1).reshape(256, 2304)  # [co][tap][ci]
    _chk("c", st["c"], xs_k @ wc.t() / 49 + p[f"{P}.support_set_cls_conv.0.bias"], xs_k.abs() @ wc.abs().t() / 49 + p[f"{P}.support_set_cls_conv.0.bias"].abs(), 2304 + 3)
    if kw["has_bias"]:
        wb = R.rbf(p[f"{P}.support_set_cls_bias.0.weight"]).permute(0, 2, 3, 1).reshape(2304)
        bb = p[f"{P}.support_set_cls_bias.0.bias"]
        _chk("rb", st["rb"], xs_k @ wb / 49 + bb, xs_k.abs() @ wb.abs() / 49 + bb.abs(), 2304 + 3)
    segs = list(seg_len)
    smax = max(segs)
    _chk("code_raw", st["code_raw"], torch.stack([t.mean(0) for t in st["c"].split(segs)]), torch.stack([t.abs().mean(0) for t in st["c"].split(segs)]), smax + 1)
    if kw["has_bias"]:
        _chk("bias_raw", st["bias_raw"], torch.stack([t.mean() for t in st["rb"].split(segs)]), torch.stack([t.abs().mean() for t in st["rb"].split(segs)]), smax + 1)
    else:
        assert float(st["bias_raw"].abs().max()) == 0
    # ---- the tail, forward and backward, from the exported code_raw (float64 formulas and their absolute-value twins)
    v0 = st["code_raw"]
    cs = p[f"{P}.conv_scale.scale"] if f"{P}.conv_scale.scale" in p else torch.ones(1, dtype=torch.float64)
    v1, a1 = v0, v0.abs()
    if kw["post_norm"]:
        pg, pb = p[f"{P}.post_norm.weight"], p[f"{P}.post_norm.bias"]
        gm = v0.reshape(n_seg, 32, 8)
        m_, r_ = gm.mean(2, keepdim=True), 1.0 / torch.sqrt(gm.var(2, unbiased=False, keepdim=True) + 1e-5)
        xh = ((gm - m_) * r_).reshape(n_seg, 256)
        axh = ((gm.abs() + m_.abs()) * r_).reshape(n_seg, 256)
        v1, a1 = xh * pg + pb, axh * pg.abs() + pb.abs()
    nrm = v1.norm(dim=1, keepdim=True).clamp_min(1e-12) if kw["conv_l2_norm"] else torch.ones(n_seg, 1, dtype=torch.float64)
    v2, a2 = v1 / nrm, a1 / nrm
    T = 256 + 32  # the L2 sum plus the GroupNorm / scale chain
    _chk("codes", codes[:, :256], v2 * cs, a2 * cs.abs(), T)
    bs = p[f"{P}.bias_scale.scale"] if kw["has_bias"] else torch.ones(1, dtype=torch.float64)
    _chk("bias", codes[:, 256], st["bias_raw"] * bs + R.prior(), (st["bias_raw"] * bs).abs() + abs(R.prior()), 3)
    Gc, Gb = G[:, :256].double(), G[:, 256].double()
    if f"{P}.conv_scale.scale" in p:
        _chk("d conv_scale", grads[f"{P}.conv_scale.scale"], (Gc * v2).sum().reshape(1), (Gc.abs() * a2).sum().reshape(1), T + 256 * n_seg)
    dv2, adv2 = Gc * cs, Gc.abs() * cs.abs()
    dv1, adv1 = dv2, adv2
    if kw["conv_l2_norm"]:
        dv1 = (dv2 - v2 * (dv2 * v2).sum(1, keepdim=True)) / nrm
        adv1 = (adv2 + a2 * (adv2 * a2).sum(1, keepdim=True)) / nrm
    dv0, adv0 = dv1, adv1
    if kw["post_norm"]:
        _chk("d post_norm.weight", grads[f"{P}.post_norm.weight"], (dv1 * xh).sum(0), (adv1 * axh).sum(0), 3 * T + n_seg + 16)
        _chk("d post_norm.bias", grads[f"{P}.post_norm.bias"], dv1.sum(0), adv1.sum(0), 3 * T + n_seg + 16)
        dxh, adxh = (dv1 * pg).reshape(n_seg, 32, 8), (adv1 * pg.abs()).reshape(n_seg, 32, 8)
        xg, axg = xh.reshape(n_seg, 32, 8), axh.reshape(n_seg, 32, 8)
        dv0 = (r_ * (dxh - dxh.mean(2, keepdim=True) - xg * (dxh * xg).mean(2, keepdim=True))).reshape(n_seg, 256)
        adv0 = (r_ * (adxh + adxh.mean(2, keepdim=True) + axg * (adxh * axg).mean(2, keepdim=True))).reshape(n_seg, 256)
    _chk("d code_raw", st["d_code_raw"], dv0, adv0, 3 * T + 64)
    lens = torch.tensor(segs, dtype=torch.float64)
    _chk("d c", st["d_c"], (st["d_code_raw"] / lens[:, None]).repeat_interleave(torch.tensor(segs), dim=0),
         (st["d_code_raw"].abs() / lens[:, None]).repeat_interleave(torch.tensor(segs), dim=0), 1)
    if kw["has_bias"]:
        _chk("d bias_scale", grads[f"{P}.bias_scale.scale"], (Gb * st["bias_raw"]).sum().reshape(1), (Gb * st["bias_raw"]).abs().sum().reshape(1), n_seg + 1)
        _chk("d bias_raw", st["d_bias_raw"], Gb * bs, (Gb * bs).abs(), 1)
        _chk("d rb", st["d_rb"], (st["d_bias_raw"] / lens).repeat_interleave(torch.tensor(segs)), (st["d_bias_raw"].abs() / lens).repeat_interleave(torch.tensor(segs)), 1)
    else:
        assert float(st["d_bias_raw"].abs().max()) == 0 and float(st["d_rb"].abs().max()) == 0
    # ---- the heads
    dc, drb = st["d_c"], st["d_rb"]
    to_w = lambda t, co: t.reshape(co, 9, 256).permute(0, 2, 1).reshape(co, 256, 3, 3)
    _chk("d cls_conv.weight", grads[f"{P}.support_set_cls_conv.0.weight"], to_w(dc.t() @ xs_k / 49, 256), to_w(dc.abs().t() @ xs_k.abs() / 49, 256), M + 2)
    _chk("d cls_conv.bias", grads[f"{P}.support_set_cls_conv.0.bias"], dc.sum(0), dc.abs().sum(0), M)
    if kw["has_bias"]:
        _chk("d cls_bias.weight", grads[f"{P}.support_set_cls_bias.0.weight"], to_w((drb @ xs_k / 49)[None], 1), to_w((drb.abs() @ xs_k.abs() / 49)[None], 1), M + 2)
        _chk("d cls_bias.bias", grads[f"{P}.support_set_cls_bias.0.bias"], drb.sum().reshape(1), drb.abs().sum().reshape(1), M)
    if L:
        dxs, adxs = dc @ wc, dc.abs() @ wc.abs()
        if kw["has_bias"]:
            dxs, adxs = dxs + drb[:, None] * wb[None], adxs + drb.abs()[:, None] * wb.abs()[None]
        _chk("d xsum", st["d_xsum"], dxs / 49, adxs / 49, 256 + 3)
        dk = st["d_xsum"].reshape(M, 9, 256)

        def scat(k):  # d x_L[q] = sum of d Xsum[tap] over the taps whose box holds q
            out = torch.zeros(M, 256, 7, 7, dtype=torch.float64)
            for t in range(9):
                out[:, :, _BOX[t // 3], _BOX[t % 3]] += k[:, t, :, None, None]
            return out
        _chk(f"d x{L}", st[f"d_x{L}"], _rows(scat(dk)), _rows(scat(dk.abs())), 9)
    # ---- the tower, backward
    R49 = M * 49
    for i in range(L - 1, -1, -1):
        ga = p[f"{P}.support_set_shared_tower.{3 * i + 1}.weight"].view(1, -1, 1, 1)
        y, xn, dxn = _maps(st[f"y{i}"]), _maps(st[f"x{i + 1}"]), _maps(st[f"d_x{i + 1}"])
        sm, sr = (ex(st[f"stats{i}"][..., j].repeat_interleave(8, dim=1)) for j in (0, 1))
        g_ = dxn * (xn > 0)
        xh_, axh_ = (y - sm) * sr, (y.abs() + sm.abs()) * sr
        grp = lambda t: t.reshape(M, 32, -1).sum(2).repeat_interleave(8, dim=1)[:, :, None, None] / 392
        dy = sr * (g_ * ga - grp(g_ * ga) - xh_ * grp(g_ * ga * xh_))
        ady = sr * ((g_ * ga).abs() + grp((g_ * ga).abs()) + axh_ * grp((g_ * ga).abs() * axh_))
        _chk(f"d y{i}", st[f"d_y{i}"], _rows(dy), _rows(ady), 392 + 16)
        _chk(f"d gamma{i}", grads[f"{P}.support_set_shared_tower.{3 * i + 1}.weight"], (g_ * xh_).sum((0, 2, 3)), (g_.abs() * axh_).sum((0, 2, 3)), R49 + 4)
        _chk(f"d beta{i}", grads[f"{P}.support_set_shared_tower.{3 * i + 1}.bias"], g_.sum((0, 2, 3)), g_.abs().sum((0, 2, 3)), R49)
        dyk = _maps(st[f"d_y{i}"])
        _chk(f"d b{i}", grads[f"{P}.support_set_shared_tower.{3 * i}.bias"], dyk.sum((0, 2, 3)), dyk.abs().sum((0, 2, 3)), R49)
        dyr = R.rbf(dyk)
        shape = (256, 256, 3, 3)
        _chk(f"d W{i}", grads[f"{P}.support_set_shared_tower.{3 * i}.weight"], torch.nn.grad.conv2d_weight(xs[i], shape, dyr, padding=1),
             torch.nn.grad.conv2d_weight(xs[i].abs(), shape, dyr.abs(), padding=1), R49 + 8)
        if i > 0:
            w = R.rbf(p[f"{P}.support_set_shared_tower.{3 * i}.weight"])
            _chk(f"d x{i}", st[f"d_x{i}"], _rows(torch.nn.grad.conv2d_input(xs[i].shape, w, dyr, padding=1)),
                 _rows(torch.nn.grad.conv2d_input(xs[i].shape, w.abs(), dyr.abs(), padding=1)), 2304)
    return codes, grad, st


SHAPES = {1: ([0], [1]), 6: ([4, 1, 7, 2, 0, 5], [2, 2, 2]), 11: (list(range(11)), [1, 3, 7]),
          44: ([(7 * i) % 9 for i in range(44)], [11, 11, 11, 11])}


@pytest.fixture(scope="module")
def eng2():
    eng = _engine()
    yield eng
    eng.close()


# ------------------------------------------------------------------------------------------------ 4: stage by stage
@pytest.mark.parametrize("M", [1, 6, 11, 44])
def test_gradient_stage_by_stage(eng2, M):
    idx, seg_len = SHAPES[M]
    rows = _bank(12, seed=M).cuda()
    if M == 44:
        shp = eng2.codegen_train_shape(44, 4)
        assert len(set(idx)) < len(idx), "repeated bank indices"
        assert shp["units"] == 11 and shp["passes"] == 2, "the weight gradient spans several units and more than one reduce pass"
    if M == 11:
        assert 11 * 49 == 539 and 539 % 32 != 0
    _stage_check(eng2, _kw(2, True, True, True), rows, idx, seg_len)


@pytest.mark.parametrize("depth", [0, 1, 2])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("bias", [True, False])
def test_gradient_stages_of_every_config(depth, variant, bias):
    eng = _engine(depth, variant[0], variant[1], bias)
    try:
        lay = eng.codegen_params()
        assert [k for k, _, _ in lay] == R.layout_keys(depth, bias, variant[0], variant[1])
        idx, seg_len = SHAPES[6]
        codes, grad, _ = _stage_check(eng, _kw(depth, variant[0], variant[1], bias), _bank(12, seed=6).cuda(), idx, seg_len)
        if not bias:
            assert torch.equal(codes[:, 256].cpu(), torch.full((3,), R.prior(), dtype=torch.float32))
        assert grad.numel() == lay[-1][1] + lay[-1][2] and bool(torch.isfinite(grad).all())
    finally:
        eng.close()


def test_zero_upstream_gradient_gives_exact_zeros(eng2):
    """a tensor that receives no gradient holds exact zeros: with d loss / d bias alone, everything behind the code does"""
    flat, lay = _params(eng2)
    idx, seg_len = SHAPES[6]
    eng2.codegen_train_forward(flat.cuda(), _bank(12, seed=6).cuda(), idx, seg_len)
    G = torch.zeros(3, 257)
    G[:, 256] = 1.0
    grad = _unflat(eng2.codegen_train_backward(G.cuda()).cpu(), lay)
    for k in (f"{P}.support_set_cls_conv.0.weight", f"{P}.support_set_cls_conv.0.bias", f"{P}.post_norm.weight", f"{P}.post_norm.bias", f"{P}.conv_scale.scale"):
        assert float(grad[k].abs().max()) == 0.0, k
    assert float(grad[f"{P}.support_set_cls_bias.0.weight"].abs().max()) > 0 and float(grad[f"{P}.support_set_shared_tower.0.weight"].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 5: end to end against float64
def test_gradient_end_to_end_against_float64(eng2, golden_dir):
    """Case 1's 3 x 4 episode.  Per tensor of at least 256 elements err = |g - g64| / |g64| for the device and for the CPU emulation (the
    restatement with the kernels' forward roundings, pinned to the reference by the CPU tests); the device's must be at most twice the
    emulation's: the factor pays for fp32 accumulation order and the gradient's own bf16 roundings of d y."""
    g = np.load(os.path.join(golden_dir, "g14_codegen_train.npz"))
    maps = torch.from_numpy(g["c3s4_maps_q8"].astype(np.float64) / 32.0)
    kw = _kw(2, True, True, True)
    sd = {k: v.double() for k, v in _gen_sd(2).items()}
    Gc, Gb = torch.from_numpy(g["c3s4_G"]), torch.from_numpy(g["c3s4_Gb"])
    _, _, sv = R.forward(maps, sd, [4, 4, 4], **kw)
    g64 = R.backward(sd, sv, Gc, Gb, **kw)
    _, _, sv = R.forward(maps, sd, [4, 4, 4], rounding=True, **kw)
    emu = R.backward(sd, sv, Gc, Gb, **kw)
    flat, lay = _params(eng2)
    rows = maps.permute(0, 2, 3, 1).reshape(12, 49, 256).to(torch.bfloat16).contiguous().cuda()
    assert torch.equal(rows.double().cpu().reshape(12, 7, 7, 256).permute(0, 3, 1, 2), maps), "the maps are bf16 values"
    eng2.codegen_train_forward(flat.cuda(), rows, list(range(12)), [4, 4, 4])
    got = _unflat(eng2.codegen_train_backward(torch.cat([Gc, Gb[:, None]], 1).float().cuda()).double().cpu(), lay)
    n = 0
    for k, _, cnt in lay:
        if cnt < 256:
            continue
        ref = g64[k].reshape(-1)
        assert float(ref.norm()) > 1e-4, k
        e_dev = float((got[k].reshape(-1) - ref).norm() / ref.norm())
        e_emu = float((emu[k].reshape(-1) - ref).norm() / ref.norm())
        print(f"{k.split('head.')[1]:45s} device {e_dev:.3e}  emulation {e_emu:.3e}")
        assert e_dev <= 2 * e_emu, k
        n += 1
    assert n == 13


# ------------------------------------------------------------------------------------------------ 6: same bits
def test_same_bits_twice_and_on_any_grid(eng2, monkeypatch):
    flat, _ = _params(eng2)
    idx, seg_len = SHAPES[44]
    rows = _bank(12, seed=44).cuda()
    G = torch.randn(4, 257, generator=torch.Generator().manual_seed(8)).cuda()
    dev = flat.cuda()
    out = []
    for cap in (None, None, "1", "3"):
        if cap is None:
            monkeypatch.delenv("SYLPH_CODEGEN_TRAIN_BLOCKS", raising=False)
        else:
            monkeypatch.setenv("SYLPH_CODEGEN_TRAIN_BLOCKS", cap)
        codes = eng2.codegen_train_forward(dev, rows, idx, seg_len).clone()
        out.append((codes, eng2.codegen_train_backward(G).clone()))
    for c, g in out[1:]:
        assert torch.equal(c, out[0][0]) and torch.equal(g, out[0][1])
    assert float(out[0][1].abs().max()) > 0


def test_third_level_of_the_reduction_tree(monkeypatch):
    """A depth-1 generator, M = 257 shots over a 12-row bank (repeated indices) in 4 segments: 65 units of 4 shots, so the ordered tree of
    csrc/partial_sum.h takes three passes at fan-in 8 (65 -> 9 -> 2 -> the final kernel).  The last unit holds ONE shot, the last chunk of
    the first pass ONE partial, and the second pass reads at the second level's offset.  d W of the tower layer against the float64 sum
    of the kernel's own exported d y (rounded to bf16, as the kernel rounds it) and x, within _chk's worst-case fp32 bound of R49 + 8
    roundings -- the bound d W has in _stage_check -- and the whole flat gradient bit-equal under block caps unset, 1 and 3.
    The class-code and box-branch gradients run the same tree from the same header (fan-in 64): their third level would need more than
    4096 units, so this test is what pins the level-offset arithmetic for them too."""
    eng = _engine(1)
    try:
        M, seg_len = 257, [64, 64, 64, 65]
        idx = [(7 * i) % 12 for i in range(M)]
        shp = eng.codegen_train_shape(M, len(seg_len))
        assert shp["units"] == 65 and shp["passes"] == 3
        rows = _bank(12, seed=257).cuda()
        dev = _params(eng)[0].cuda()
        lay = eng.codegen_params()
        G = torch.randn(len(seg_len), 257, generator=torch.Generator().manual_seed(8)).cuda()
        monkeypatch.delenv("SYLPH_CODEGEN_TRAIN_BLOCKS", raising=False)
        eng.codegen_train_forward(dev, rows, idx, seg_len)
        grad, st = eng.codegen_train_backward(G, debug=True)
        grad = grad.clone()
        # d W[co][(ci, ky, kx)] = sum over rows of bf16(d y)[row][co] x[row + tap][ci]: one float64 product over the M * 49 rows
        dyr = R.rbf(_maps(st["d_y0"])).reshape(M, 256, 49).permute(1, 0, 2).reshape(256, M * 49)
        xu = F.unfold(_maps(rows.cpu()[torch.tensor(idx)]), 3, padding=1).permute(1, 0, 2).reshape(2304, M * 49)
        got = _unflat(grad.cpu(), lay)[f"{P}.support_set_shared_tower.0.weight"]
        _chk("d W0", got, dyr @ xu.t(), dyr.abs() @ xu.abs().t(), M * 49 + 8)
        for cap in ("1", "3"):
            monkeypatch.setenv("SYLPH_CODEGEN_TRAIN_BLOCKS", cap)
            eng.codegen_train_forward(dev, rows, idx, seg_len)
            assert torch.equal(eng.codegen_train_backward(G), grad), f"block cap {cap}: other bits"
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ refusals (host checks, before any launch)
def test_refusals_by_name(eng2):
    flat, _ = _params(eng2)
    dev, rows = flat.cuda(), _bank(4, seed=1).cuda()
    with pytest.raises(RuntimeError, match=r"idx\[1\] = 4 is outside the bank of 4 rows"):
        eng2.codegen_train_forward(dev, rows, [0, 4], [2])
    with pytest.raises(RuntimeError, match="sum to 3, not to M = 2"):
        eng2.codegen_train_forward(dev, rows, [0, 1], [1, 2])
    with pytest.raises(RuntimeError, match="at least one index"):
        eng2.codegen_train_forward(dev, rows, [], [1])
    from test_hip_parity import _cfg as base, _roienc_cfg
    from sylph_amd.engine import Engine
    cases = [("fp32", _cfg(), "bf16 mode only"), ("f32s", _cfg(), "bf16 mode only"), ("bf16", _roienc_cfg(), "ROIEncoder")]
    for key, val, match in (("CLS_LAYER", ["", "", 3], "3x3 class codes"), ("WEIGHT_LAYER", ["", "", 1], "WEIGHT_LAYER"), ("SCALE_LAYER", ["", "", 1], "SCALE_LAYER"),
                            ("BIAS_L2_NORM", True, "BIAS_L2_NORM"), ("TOWER_LAYERS", [["GN", "ReLU"], ["", "ReLU"]], r"TOWER_LAYERS\[1\]")):
        cfg = base()
        setattr(cfg.MODEL.META_LEARN.CODE_GENERATOR, key, val)
        cases.append(("bf16", cfg, match))
    for dtype, cfg, match in cases:
        e = Engine(cfg, dtype=dtype)
        try:
            with pytest.raises(RuntimeError, match=match):
                e.codegen_params()
            with pytest.raises(RuntimeError, match=match):
                e.codegen_train_shape(4, 2)
        finally:
            e.close()


# ------------------------------------------------------------------------------------------------ 7: install
def _support_batch(eng, B=3, hw=(64, 96), seed=3):
    from test_support_bf16_pinned_gpu import _box_sets, _pyramid
    feats = _pyramid(B, hw[0], hw[1], seed=seed)
    eng.import_pyramid(feats, hw)
    return feats, _box_sets(7, hw[0], hw[1], seed=107)[0]


ROI_IMAGE, SEG_LEN = [2, 0, 2, 2, 0, 2, 0], [3, 1, 3]


def test_install_is_bit_identical_to_a_fresh_engine():
    from sylph_amd import synthetic as W
    from sylph_amd.shots import ShotBank
    head = W.head_state_dict(seed=3)
    eng = _engine(extra=head)
    trained = _gen_sd(2, seed=9)
    from sylph_amd.engine import Engine
    other = Engine(_cfg(), dtype="bf16")
    sd = dict(head)
    sd.update(trained)
    other.load_state_dict(sd)
    try:
        _, boxes = _support_batch(eng)
        _support_batch(other)
        run = lambda e: e.normalize_codes(e.codegen_rois(boxes, ROI_IMAGE, SEG_LEN).clone())
        before = run(eng).clone()
        bank = ShotBank(eng.shot_key(), device=eng.device)
        bank.stamp = eng.codegen_stamp()
        bank.append(eng.codegen_shots(boxes, ROI_IMAGE), [0] * 7, [0] * 7, list(range(7)))
        eng.towers()
        rec = eng.store_record()
        assert eng.codegen_stamp() == 0
        flat, lay = _params(eng, trained)
        eng.set_code_generator(flat)
        assert eng.codegen_stamp() == 1
        _support_batch(eng)
        want = run(other)
        got = run(eng)
        assert torch.equal(got, want) and not torch.equal(got, before)
        assert torch.equal(eng.code_generator(), _params(eng, _gen_sd(2))[0]), "get returns the finalized tensors"
        with pytest.raises(ValueError, match="generator stamp 0, the engine now runs stamp 1"):
            bank.check_stamp(eng)
        eng.load_record(rec)  # query records stay loadable
        _support_batch(eng)
        eng.set_code_generator({k: v for k, v in trained.items()})  # the dict form; a fresh stamp
        assert eng.codegen_stamp() == 2 and torch.equal(run(eng), want)
        eng.set_code_generator(None)
        assert eng.codegen_stamp() == 0
        bank.check_stamp(eng)
        assert torch.equal(run(eng), before), "a restore gives back the original bits"
        eng.load_record(rec)
        rec.close()
    finally:
        eng.close()
        other.close()


# ------------------------------------------------------------------------------------------------ 8: training forward against the served pass
def test_training_forward_against_the_served_pass():
    """roi_rows of the ROIs, then codegen_train_forward, against codegen_rois + normalize_codes; both against the float64 oracle on the
    same bf16 pyramid.  The served pass is the yardstick: the training forward's max error is at most twice its own."""
    from oracle import codegen as OC
    from oracle.roi_align import roi_pooler
    eng = _engine()
    try:
        feats, boxes = _support_batch(eng)
        served = eng.normalize_codes(eng.codegen_rois(boxes, ROI_IMAGE, SEG_LEN).clone()).cpu().double()
        rows = eng.roi_rows(boxes, ROI_IMAGE)
        nchw = eng.roi_align_rois(boxes, ROI_IMAGE)
        assert torch.equal(rows.float().reshape(7, 7, 7, 256).permute(0, 3, 1, 2), nchw), "roi_rows holds roi_align_rois' values"
        flat, _ = _params(eng)
        train = eng.codegen_train_forward(flat.cuda(), rows, list(range(7)), SEG_LEN).cpu().double()
        sd = {k: v.double() for k, v in _gen_sd(2).items()}
        roi = torch.cat([roi_pooler([f[i:i + 1].double() for f in feats], boxes[r:r + 1].double(), (8, 16, 32, 64, 128), out_size=7)
                         for r, i in enumerate(ROI_IMAGE)])
        code, bias, _ = R.forward(roi.double(), sd, SEG_LEN, **_kw(2, True, True, True))
        want = torch.cat([code, bias[:, None]], 1)
        e_served, e_train = float((served - want).abs().max()), float((train - want).abs().max())
        print(f"max |err| against float64: served {e_served:.3e}, training forward {e_train:.3e}")
        assert e_served > 0 and e_train <= 2 * e_served
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 9: the loop
def test_train_code_generator_descends():
    """A tiny episode pool: 2 records of a 128 x 160 batch, a bank of 5 classes x 3 rows, episodes of 3 classes x 2 shots, 30 steps at
    lr 0.01 with the recipes' clipping (norm 1.0).  lr was chosen on the CPU: the float64 restatement alone (codegen_train_ref.loop_ref on
    the oracle's tower outputs) goes from 1.166 (mean of the first 5 steps) to 0.510 (last 5).  First the restatement, driven with the
    same draws on the kernel's own operand values, must descend; then the device run."""
    from sylph_amd import synthetic as W
    from sylph_amd.finetune import step_records
    from sylph_amd.metatrain import RoiBank, episode_annotations, train_code_generator
    from test_finetune_gpu import _operand
    eng = _engine(extra=W.head_state_dict(seed=3))
    eng.set_debug_taps(True)
    try:
        recs, anns, xns = [], [], []
        for feats, ann in FR.loop_task()[:2]:
            eng.import_pyramid(feats, FR.LOOP_HW)
            eng.towers()
            xns.append(_operand(eng))
            recs.append(eng.store_record())
            anns.append(ann)
        cls = [c for c in range(FR.LOOP_CLASSES) for _ in range(3)]
        rows = _bank(len(cls), seed=77)
        bank = RoiBank(eng.device).append(rows, cls)
        iters, seed = 30, 0
        eps, ins = [], []
        for it, step in enumerate(step_records(2, None, iters, seed)):
            idx, sl, cids = bank.draw(3, 2, seed + it)
            eps.append((idx, sl))
            cur = []
            for r in step:
                bx, cl, im = episode_annotations(anns[r], cids)
                cur.append((xns[r], torch.from_numpy(FR.fcos_targets_ref(bx.numpy(), cl.numpy(), im.numpy(), 2, FR.levels(FR.LOOP_HW)))))
            ins.append(cur)
        want = R.loop_ref(R.rows_to_maps(rows.double()), _gen_sd(2), eps, ins, lr=0.01, **_kw(2, True, True, True))
        state, losses = train_code_generator(eng, bank, recs, anns, iters=iters, classes_per_step=3, shots=2, lr=0.01, clip_norm=1.0, seed=seed)
        ls = losses.cpu().tolist()
        f5, l5 = lambda v: sum(v[:5]) / 5, lambda v: sum(v[-5:]) / 5
        print(f"loss, mean of the first / last 5 steps: float64 restatement {f5(want):.4f} -> {l5(want):.4f}; device {f5(ls):.4f} -> {l5(ls):.4f}")
        assert l5(want) < f5(want), "the float64 restatement descends"
        assert all(np.isfinite(ls)) and l5(ls) < f5(ls), "the device run descends"
        lay = eng.codegen_params()
        assert sorted(state) == sorted(k for k, _, _ in lay)
        for k, _, n in lay:
            assert state[k].numel() == n and state[k].dtype == torch.float32
        assert not torch.equal(state[f"{P}.support_set_cls_conv.0.weight"].reshape(-1), _gen_sd(2)[f"{P}.support_set_cls_conv.0.weight"].reshape(-1))
        for r in recs:
            r.close()
    finally:
        eng.close()
