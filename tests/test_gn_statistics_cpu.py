"""The crafted tower layer and the displacement metric of tests/gn_stats_ref.py, checked in float64 without a GPU: every output
group of the crafted conv has the distribution its name says (so that the GPU tests exercise what they claim to), and the metric
rejects coefficients whose rstd is off by 1e-3."""
import torch

import gn_stats_ref as G

H, W = 128, 160


def _layer0(seed=21):
    feats = G.crafted_pyramid(2, H, W, seed)
    w, bias = G.crafted_layer(seed + 1)
    return feats, w, bias, [G.conv_f64(x, w, bias) for x in feats]


def test_crafted_groups_have_their_distribution():
    """P3 of a 128 x 160 pyramid (16 x 20 positions, two images): measured R within 10 % of nominal (+ 0.25 absolute: the 0.1-scale
    biases and the sampling noise of the group mean, which is all an R = 0 group has), the step groups' variance almost all between
    the halves, zero-variance groups exactly 0, the constant-per-channel group exactly the variance of its biases."""
    _, w, bias, vs = _layer0()
    v = vs[0]
    got = G.measured(v, G.LAYOUT, bias)
    for gi, (kind, R, A) in enumerate(G.LAYOUT):
        m = got[gi]
        print(gi, G.label(G.LAYOUT[gi]), m)
        if kind in ("offset", "step"):
            assert abs(m["R"] - R) <= 0.1 * R + 0.25, (gi, kind, R, m)
        if kind == "offset" or kind == "control":
            assert m["step_share"] < 0.02 and 0.8 < m["var"] and m["var_max"] < 1.1, (gi, kind, m)
        if kind == "step":  # A^2 / (A^2 + sigma^2) = 64 / 65
            assert m["step_share"] > 0.98 and abs(m["var"] - 65.0) < 2.0, (gi, m)
        if kind == "purestep":
            assert m["step_share"] > 1.0 - 1e-12 and abs(m["var"] - 64.0) < 1e-9, (gi, m)
        if kind == "zerovar":
            assert m["var"] == 0.0 and m["var_max"] == 0.0, (gi, m)
            assert float((v[:, 8 * gi:8 * gi + 8] - R).abs().max()) == 0.0
        if kind == "constch":
            b = torch.tensor(G.CONSTCH_BIASES, dtype=torch.float64)
            assert abs(m["var"] - float(b.var(unbiased=False))) < 1e-12 and m["var"] == m["var_max"], (gi, m)
        if kind == "outlier":  # one input of 2^12 among unit ones: 9 taps of 320 positions carry ~2^12 / sqrt(9 * 253) = 86 sigma
            assert m["var"] > 50.0, (gi, m)
    kinds = {lay[0] for lay in G.LAYOUT}
    assert kinds == {"offset", "step", "zerovar", "constch", "outlier", "purestep", "control"} and len(G.LAYOUT) == 32
    assert sorted(r for k, r, _ in G.LAYOUT if k == "offset") == [0.0, 4.0, 16.0, 64.0, 256.0, 1024.0]
    assert float((G.bf(w) - w).abs().max()) == 0.0, "crafted weights must be exact in bf16"


def test_reference_matches_torch_group_norm():
    g = torch.Generator().manual_seed(3)
    v = torch.randn(2, 256, 5, 7, generator=g, dtype=torch.float64) * 3 + 1.5
    gamma, beta = G.gn_params(4)
    ref = G.gn_ref(v, gamma, beta)
    want = torch.nn.functional.group_norm(v, 32, gamma.double(), beta.double(), G.GN_EPS)
    assert float((G.gn_apply_f64(v, ref) - want).abs().max()) < 1e-12


def test_metric_passes_rounded_reference_and_rejects_rstd_off_by_1e_3():
    """The reference coefficients rounded to fp32 (the best any kernel can do) pass every group in every mode; the same with rstd off
    by 1e-3 relative (b formed from the same a, as the finalizer does: the normalised values are scaled about the mean, 4e-3 at
    4 sigma) fail at R = 64 and beyond in every mode."""
    _, _, bias, vs = _layer0()
    gamma, beta = G.gn_params(5)
    ref = G.gn_ref(vs[0], gamma, beta)
    exact = torch.stack([ref["a"].float(), ref["b"].float()], dim=2)
    rstd = (1.0 / ref["s"]) * (1.0 + 1e-3)
    a = (rstd.float() * gamma.view(1, -1))
    off = torch.stack([a, beta.view(1, -1) - ref["m"].float() * a], dim=2)
    for mode in ("bf16", "f32", "f32s"):
        assert G.check_coef(exact, ref, mode, G.LAYOUT, "fp32-rounded reference", "P3") == []
        bad = "\n".join(G.check_coef(off, ref, mode, G.LAYOUT, "rstd * (1 + 1e-3)", "P3"))
        for gi, (kind, R, A) in enumerate(G.LAYOUT):
            if kind in ("offset", "step") and R >= 64:
                assert f"group {gi} " in bad, (mode, gi, bad)


def test_element_bound_grows_only_beyond_four_sigma():
    g = torch.Generator().manual_seed(8)
    v = torch.randn(1, 256, 4, 4, generator=g, dtype=torch.float64)
    v[0, 0, 0, 0] = 40.0
    gamma, beta = G.gn_params(6)
    ref = G.gn_ref(v, gamma, beta)
    eb, b = G.element_bound(v, ref, "f32"), G.bound(ref, "f32")
    assert float(eb[0, 0, 0, 0]) > float(b[0, 0]) and float(eb[0, 9, 1, 1]) == float(b[0, 9])
