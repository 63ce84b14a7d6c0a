"""The bounds of tests/test_support_bf16_pinned_gpu.py have teeth: for each stage, the unperturbed restatement evaluated in fp32 in
another order passes the bound the GPU test holds the kernel to, and a perturbation of the kind a subtly wrong kernel makes fails it
(as tests/test_bf16_ulps_cpu.py does for the single-conv bound)."""
import math

import numpy as np
import pytest
import torch

from bf16_ulps import assert_f32, assert_tail, assert_ulps, bf16_rne, codegen_tail_f64
from independent_refs import _axis_weights, level_of_box, roi_pool_separable_f64

STRIDES = (8, 16, 32, 64, 128)
H, W = 128, 192


def _pyramid(S=3, seed=5):
    from oracle import bf16 as B
    g = torch.Generator().manual_seed(seed)
    return [B.r(torch.randn(S, 256, h, w, generator=g)) for h, w in ((16, 24), (8, 12), (4, 6), (2, 3), (1, 2))]


BOXES = torch.tensor([[10.0, 12.0, 130.0, 100.0], [-20.0, 30.0, 60.0, 150.0], [40.0, 5.0, 190.0, 120.0]])  # bins of 2 x 2 samples or more


def _pool_one(feat, box, level, shift=0.5):
    """float64 ROIAlign of one box on one level; shift = 0.5: aligned (the -0.5 pixel shift), 0: aligned=False."""
    sc = 1.0 / STRIDES[level]
    x1, y1, x2, y2 = (float(v) * sc - shift for v in box)
    Ay = _axis_weights(y1, y2 - y1, feat.shape[1])
    Ax = _axis_weights(x1, x2 - x1, feat.shape[2])
    return np.einsum("ph,chw,qw->cpq", Ay, np.asarray(feat, dtype=np.float64), Ax)


def _roi_reference(feats):
    return bf16_rne(torch.from_numpy(roi_pool_separable_f64([f.numpy() for f in feats], BOXES.numpy(), f32_coords=True)))


def _roi_perturbed(feats, how):
    ref = roi_pool_separable_f64([f.numpy() for f in feats], BOXES.numpy(), f32_coords=True)
    i = 0
    lvl = level_of_box(BOXES[i].tolist()) - 3
    f = feats[lvl][i].double().numpy()
    if how == "aligned_false":
        ref[i] = _pool_one(f, BOXES[i], lvl, shift=0.0)
    elif how == "neighbour_level":
        ref[i] = _pool_one(feats[lvl + 1][i].double().numpy(), BOXES[i], lvl + 1)
    elif how == "dropped_sample":  # bin (3, 3) without its first sample point
        sc = 1.0 / STRIDES[lvl]
        x1, y1, x2, y2 = (float(v) * sc - 0.5 for v in BOXES[i])
        bh, bw = (y2 - y1) / 7, (x2 - x1) / 7
        gh, gw = math.ceil(bh), math.ceil(bw)
        assert gh * gw >= 4
        yy, xx = y1 + 3 * bh + 0.5 * bh / gh, x1 + 3 * bw + 0.5 * bw / gw
        y0, x0 = int(yy), int(xx)  # inside the map: plain bilinear
        ly, lx = yy - y0, xx - x0
        s = ((1 - ly) * (1 - lx) * f[:, y0, x0] + (1 - ly) * lx * f[:, y0, x0 + 1] + ly * (1 - lx) * f[:, y0 + 1, x0]
             + ly * lx * f[:, y0 + 1, x0 + 1])
        ref[i, :, 3, 3] -= s / (gh * gw)
    return bf16_rne(torch.from_numpy(ref))


def test_roi_fp32_restatement_passes():
    from oracle import bf16 as B
    feats = _pyramid()
    assert_ulps(B.roi_pool(feats, BOXES), _roi_reference(feats), "fp32 sample-by-sample ROIAlign")


@pytest.mark.parametrize("how", ["dropped_sample", "aligned_false", "neighbour_level"])
def test_roi_perturbation_fails(how):
    feats = _pyramid()
    with pytest.raises(AssertionError):
        assert_ulps(_roi_perturbed(feats, how), _roi_reference(feats), how)


# ---- GroupNorm statistics ------------------------------------------------------------------------------------------
def _gn_operands():
    g = torch.Generator().manual_seed(7)
    v = torch.randn(2, 256, 7, 7, generator=g) * (1 + torch.rand(1, 256, 1, 1, generator=g)) + 0.3 * torch.randn(2, 256, 1, 1, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(256, generator=g), 0.1 * torch.randn(256, generator=g)
    return v, gamma, beta


def test_gn_fp32_statistics_pass():
    from oracle import bf16 as B
    v, gamma, beta = _gn_operands()
    x = v.reshape(2, 32, -1).flip(2)  # fp32, another order
    mean = x.mean(dim=2)
    var = ((x - mean.unsqueeze(2)) ** 2).mean(dim=2)
    a = (gamma.view(1, 32, 8) / torch.sqrt(var + 1e-5).unsqueeze(2)).reshape(2, 256)
    b = beta.view(1, 256) - mean.repeat_interleave(8, dim=1) * a
    assert_f32(torch.stack([a, b], dim=2), B.gn_coef(v.double(), gamma, beta), "fp32 GroupNorm coefficients")


def test_gn_statistics_straddling_the_next_image_fail():
    """Image 0's statistics over its 49 positions and the first 16 rows of image 1 (a tile or patch pair across the boundary)."""
    from oracle import bf16 as B
    v, gamma, beta = _gn_operands()
    rows0, rows1 = v[0].reshape(256, 49), v[1].reshape(256, 49)
    both = torch.cat([rows0, rows1[:, :16]], dim=1).reshape(1, 256, 65, 1)
    bad = torch.cat([B.gn_coef(both.double(), gamma, beta), B.gn_coef(v[1:].double(), gamma, beta)])
    with pytest.raises(AssertionError):
        assert_f32(bad, B.gn_coef(v.double(), gamma, beta), "straddled statistics")


# ---- codegen tail ---------------------------------------------------------------------------------------------------
def _tail_operands(shots=5, ncls=2):
    g = torch.Generator().manual_seed(9)
    S = shots * ncls
    conv = torch.randn(S, 256, 7, 7, generator=g) + 0.2
    bias = torch.randn(S, 1, 7, 7, generator=g)
    wl = torch.randn(S, 1, 7, 7, generator=g) + torch.randn(S, 1, 1, 1, generator=g)
    sc = torch.randn(S, 1, 7, 7, generator=g) + 1
    return conv, bias, wl, sc, shots


@pytest.mark.parametrize("weighted", [False, True])
def test_tail_fp32_restatement_passes(weighted):
    from oracle import bf16 as B
    conv, bias, wl, sc, shots = _tail_operands()
    w = (wl, sc) if weighted else (None, None)
    want, _, tol = codegen_tail_f64(conv, bias, shots, *w, bias_l2_norm=weighted)
    got, _ = B.codegen_tail(conv.flip(3), bias.flip(3), shots, *[t.flip(3) if t is not None else None for t in w], bias_l2_norm=weighted)
    assert_tail(got, want, tol, "fp32 tail, positions reversed")


def test_tail_without_the_49th_position_fails():
    from oracle import bf16 as B
    conv, bias, wl, sc, shots = _tail_operands()
    want, _, tol = codegen_tail_f64(conv, bias, shots)
    c48 = conv.flatten(2)[:, :, :48].reshape(-1, 256, 48, 1)
    b48 = bias.flatten(2)[:, :, :48].reshape(-1, 1, 48, 1)
    got, _ = B.codegen_tail(c48, b48, shots)
    with pytest.raises(AssertionError):
        assert_tail(got, want, tol, "48 positions")


def test_tail_with_two_softmax_weights_swapped_fails():
    from oracle import bf16 as B
    conv, bias, wl, sc, shots = _tail_operands()
    want, _, tol = codegen_tail_f64(conv, bias, shots, wl, sc, bias_l2_norm=True)
    perm = torch.arange(conv.shape[0])
    perm[0], perm[1] = 1, 0  # shot 0 takes shot 1's weight and the other way round
    got, _ = B.codegen_tail(conv, bias, shots, wl[perm], sc, bias_l2_norm=True)
    with pytest.raises(AssertionError):
        assert_tail(got, want, tol, "swapped shot weights")


# ---- ROIEncoder token stack -----------------------------------------------------------------------------------------
def _token_operands(S=40):
    from oracle import bf16 as B
    from sylph_amd import synthetic as Wt
    g = torch.Generator().manual_seed(11)
    x = B.r(torch.relu(torch.randn(S, 256, 7, 7, generator=g)))
    return x, Wt.roi_encoder_state_dict(seed=4)


def test_tokenizer_fc_fp32_passes():
    from oracle import bf16 as B
    x, sd = _token_operands()
    want = B.tokenizer_fc(x.double(), {k: v.double() for k, v in sd.items()})
    assert_f32(B.tokenizer_fc(x, sd), want, "fp32 tokenizer FCs")


def test_tokenizer_fc_channel_major_read_fails():
    from oracle import bf16 as B
    x, sd = _token_operands()
    want = B.tokenizer_fc(x.double(), {k: v.double() for k, v in sd.items()})
    with pytest.raises(AssertionError):
        assert_f32(B.tokenizer_fc(x, sd, position_major=True), want, "activations read in the other order")


def test_linear_second_row_group_reading_the_first_fails():
    """linear_kernel's 16-row groups: rows 16..31 computed from rows 0..15."""
    x, sd = _token_operands()
    t = x.flatten(1)
    wt, b = sd["code_generator.tokenizer.fc1.weight"], sd["code_generator.tokenizer.fc1.bias"]
    want = torch.nn.functional.linear(t.double(), wt.double(), b.double())
    assert_f32(torch.nn.functional.linear(t, wt, b), want, "fp32 linear")
    bad = torch.nn.functional.linear(torch.cat([t[:16], t[:16], t[32:]]), wt, b)
    with pytest.raises(AssertionError):
        assert_f32(bad, want, "second row group reads the first")
