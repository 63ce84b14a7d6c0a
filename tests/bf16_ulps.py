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
    mag = torch.maximum(torch.maximum(got.abs(), want.abs()), torch.full_like(want, fl))
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
