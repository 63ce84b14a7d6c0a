"""bf16-ulp comparison helpers shared by the ulp-level GPU tests (tests/test_bf16_pinned_gpu.py, tests/test_conv_routes_gpu.py), and
the float64 single-conv reference they are held against.  The bounds themselves are stated in those files' docstrings."""
import numpy as np
import torch
import torch.nn.functional as F


def ulps(got, want, floor="max"):
    """(fraction of elements not bit-identical, worst difference in bf16 ulps).  The ulp of an element is taken at
    max(|element|, floor) with floor = 1e-3 * max|want| ("max": single-conv kernels) or rms(want) ("rms": chains of convs
    with bf16 intermediates; see tests/test_bf16_pinned_gpu.py)."""
    got, want = got.float().cpu(), want.float().cpu()
    diff = (got - want).abs()
    fl = 1e-3 * float(want.abs().max()) if floor == "max" else float(want.pow(2).mean().sqrt())
    mag = torch.maximum(torch.maximum(got.abs(), want.abs()), torch.full_like(want, fl)).clamp_min(2.0 ** -126)  # all-zero tensors
    ulp = torch.exp2(torch.floor(torch.log2(mag)) - 7)
    return float((diff > 0).float().mean()), float((diff / ulp).max())


def assert_ulps(got, want, what, max_ulp=1.0, max_frac=0.01, floor="max"):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    frac, worst = ulps(got, want, floor)
    print(f"{what}: {frac * 100:.3f} % of elements differ, worst {worst:.2f} bf16 ulp")
    assert worst <= max_ulp and frac <= max_frac, f"{what}: {frac:.4f} of elements differ, worst {worst:.2f} ulp"


def assert_chain(got, want, what, max_ulp=16.0, max_rel_l2=2.0 ** -8):
    """Chains of blocks (tests/test_bf16_pinned_gpu.py): error energy and worst element."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    frac, worst = ulps(got, want, "rms")
    g, w = got.float().cpu(), want.float().cpu()
    rel = float((g - w).pow(2).sum().sqrt() / w.pow(2).sum().sqrt())
    print(f"{what}: relative L2 error {rel:.2e}, {frac * 100:.1f} % of elements differ, worst {worst:.2f} bf16 ulp")
    assert rel <= max_rel_l2 and worst <= max_ulp, f"{what}: relative L2 {rel:.3e}, worst {worst:.2f} ulp"


def bf16_rne(t):
    """Round a float64 tensor to bf16, round-to-nearest-even, in ONE step (torch's float64 -> bfloat16 goes through float32: a double
    rounding), returned as float32.  Finite values in the normal bf16 range; zeros stay zeros."""
    a = t.detach().cpu().double().contiguous().numpy().view(np.int64).copy()
    lsb = (a >> 45) & 1
    a = (a + ((1 << 44) - 1) + lsb) & ~np.int64((1 << 45) - 1)
    return torch.from_numpy(a.view(np.float64)).float()


def conv_epilogue_f64(x, w, scale, shift, stride=1, pad=0, relu=False, res=None):
    """conv2d(x, w) * scale + shift (+ res), then ReLU, all in float64 on the CPU (x, w, res as given: the caller rounds them to
    bf16 when the kernel stores bf16 operands)."""
    acc = F.conv2d(x.double().cpu(), w.double().cpu(), None, stride, pad)
    y = acc * scale.double().cpu().view(1, -1, 1, 1) + shift.double().cpu().view(1, -1, 1, 1)
    if res is not None:
        y = y + res.double().cpu()
    return F.relu(y) if relu else y


def assert_f32(got, want, what, rel=1e-4):
    """fp32 outputs: max |difference| <= rel * max(1, max |want|) (summation order; tests/test_bf16_pinned_gpu.py)."""
    got, want = got.float().cpu(), want.float().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float((got - want).abs().max())
    scale = max(1.0, float(want.abs().max()))
    print(f"{what}: max |diff| {err:.3e} (scale {scale:.3f})")
    assert err <= rel * scale, f"{what}: max |diff| {err} > {rel} * {scale}"


U32 = 2.0 ** -24


def codegen_tail_f64(conv_out, bias_map, shots, weight_map=None, scale_map=None, bias_l2_norm=False):
    """codegen_tail_kernel in float64 from its fp32 inputs (S, C, 7, 7) -> (codes (classes, C + 1), cls_weight_norm or None, and the
    per-element error bound of an fp32 evaluation, (classes, C + 1)).

    Bound (u = 2^-24): a position mean is a recursive fp32 sum of 49 terms and one division, <= (49 + 1) u sum|x| / 49 per shot; the
    shot combination adds S products and sums, (S + 2) u relative to sum_s w_s |pool_s|.  Softmax shot weights (WEIGHT_LAYER) carry the
    error of their pooled logit, <= 50 u mean|l| absolute, through exp and the normalisation (+ 8 u relative): |dw_s| <= w_s (100 u
    max_s mean|l_s| + 8 u), weighted by |pool_s|.  BIAS_L2_NORM divides by a 49-term fp32 norm (<= 52 u relative)."""
    x = conv_out.double().flatten(2)
    S, C, npos = x.shape
    ncls = S // shots
    pooled = x.mean(dim=2).view(ncls, shots, C)
    absm = x.abs().mean(dim=2).view(ncls, shots, C)
    dw = torch.zeros(ncls, shots, dtype=torch.float64)
    if weight_map is not None:
        lg = weight_map.double().flatten(1)
        w = torch.softmax(lg.mean(dim=1).view(ncls, shots), dim=1)
        dw = w * (100 * U32 * lg.abs().mean(dim=1).view(ncls, shots).amax(dim=1, keepdim=True) + 8 * U32)
    else:
        w = torch.full((ncls, shots), 1.0 / shots, dtype=torch.float64)
    codes = torch.zeros(ncls, C + 1, dtype=torch.float64)
    tol = torch.zeros(ncls, C + 1, dtype=torch.float64)
    codes[:, :C] = (w.unsqueeze(2) * pooled).sum(dim=1)
    tol[:, :C] = (50 + shots + 2) * U32 * (w.unsqueeze(2) * absm).sum(dim=1) + (dw.unsqueeze(2) * pooled.abs()).sum(dim=1)
    if bias_map is not None:
        bm = bias_map.double().flatten(1)
        relerr = 50 * U32
        if bias_l2_norm:
            bm = bm / bm.norm(dim=1, keepdim=True).clamp_min(1e-12)
            relerr += 52 * U32
        bp = bm.mean(dim=1).view(ncls, shots)
        codes[:, C] = (w * bp).sum(dim=1)
        tol[:, C] = (relerr + (shots + 2) * U32) * (w * bm.abs().mean(dim=1).view(ncls, shots)).sum(dim=1) + (dw * bp.abs()).sum(dim=1)
    wn = None
    if scale_map is not None:
        sp = scale_map.double().flatten(1).mean(dim=1).view(ncls, shots)
        wn = (w * sp).sum(dim=1)
    return codes, wn, tol


def assert_tail(got, want, tol, what):
    got, want = got.double().cpu(), want.double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    excess = float(((got - want).abs() / tol.clamp_min(1e-30)).max())
    print(f"{what}: worst |diff| / fp32 bound {excess:.3f}")
    assert excess <= 1.0, f"{what}: an element is {excess:.2f} x its fp32 summation bound away"
