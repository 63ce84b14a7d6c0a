"""The bf16-ulp bound of the single-conv tests (tests/bf16_ulps.py: worst element <= 1 ulp with the floor at 1e-3 of the tensor
maximum, <= 1 % of elements not identical) has teeth: a float64 conv reference rounded once to bf16 (RNE) passes against itself
re-summed in fp32 in another order, and fails against four perturbations of the kind a subtly wrong kernel makes."""
import pytest
import torch
import torch.nn.functional as F

from bf16_ulps import assert_ulps, bf16_rne, conv_epilogue_f64

B, CIN, COUT, H, W = 2, 64, 48, 16, 16  # 512 output rows: four 128-row tiles; two 32-channel K-slices


def _operands():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, CIN, H, W, generator=g).bfloat16().float()
    w = (torch.randn(COUT, CIN, 3, 3, generator=g) / (CIN * 9) ** 0.5).bfloat16().float()
    scale = torch.rand(COUT, generator=g) + 0.5
    shift = torch.randn(COUT, generator=g) * 0.1
    return x, w, scale, shift


def _reference():
    x, w, scale, shift = _operands()
    return bf16_rne(conv_epilogue_f64(x, w, scale, shift, 1, 1, True))


def test_bf16_rne_is_one_rounding():
    t = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40, -(1.0 + 2.0 ** -8 + 2.0 ** -40), 0.0, 3.0],
                     dtype=torch.float64)  # float32 would already have rounded the third and fourth to the tie
    assert bf16_rne(t).tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -(1.0 + 2.0 ** -7), 0.0, 3.0]
    r = torch.randn(10000)  # float32 values: torch's float32 -> bfloat16 is a single RNE rounding
    assert torch.equal(bf16_rne(r.double()), r.bfloat16().float())


def test_fp32_resummed_reference_passes():
    """The kernels sum in fp32 in their own order: the float64 reference re-summed in fp32 over the K-slices in reverse order,
    epilogue in fp32, one bf16 RNE rounding, is within the bound."""
    x, w, scale, shift = _operands()
    acc = torch.zeros(B, COUT, H, W)
    for k0 in reversed(range(0, CIN, 32)):
        acc = acc + F.conv2d(x[:, k0:k0 + 32], w[:, k0:k0 + 32], None, 1, 1)
    got = F.relu(acc * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)).bfloat16().float()
    assert_ulps(got, _reference(), "fp32 re-summed")


def _truncated():
    x, w, scale, shift = _operands()
    y = conv_epilogue_f64(x, w, scale, shift, 1, 1, True)
    a = y.numpy().view("int64") & ~((1 << 45) - 1)
    return torch.from_numpy(a.view("float64")).float()


def _neighbour_scale():
    x, w, scale, shift = _operands()
    s = scale.clone()
    s[COUT - 1] = scale[COUT - 2]  # the last real channel reads its neighbour's scale
    return bf16_rne(conv_epilogue_f64(x, w, s, shift, 1, 1, True))


def _dropped_k_slice():
    """Output rows 128..255 (the second 128-row tile) without input channels 32..63."""
    x, w, scale, shift = _operands()
    full = conv_epilogue_f64(x, w, scale, shift, 1, 1, True)
    xd = x.clone()
    xd[:, 32:] = 0
    part = conv_epilogue_f64(xd, w, scale, shift, 1, 1, True)
    f, p = full.permute(0, 2, 3, 1).reshape(-1, COUT), part.permute(0, 2, 3, 1).reshape(-1, COUT)
    f[128:256] = p[128:256]
    return bf16_rne(f.reshape(B, H, W, COUT).permute(0, 3, 1, 2))


def _shifted_tap():
    """Tap (ky = 2, kx = 1) reads input row y instead of y + 1 for the output rows at the lower edge of 8-row patches."""
    x, w, scale, shift = _operands()
    acc = F.conv2d(x.double(), w.double(), None, 1, 1)
    diff = torch.zeros_like(x.double())
    diff[:, :, :-1] = x.double()[:, :, :-1] - x.double()[:, :, 1:]
    delta = F.conv2d(diff, w.double()[:, :, 2:3, 1:2])
    rows = torch.arange(H) % 8 == 7
    rows[H - 1] = False  # the tap reads the zero pad there
    acc[:, :, rows] += delta[:, :, rows]
    y = F.relu(acc * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1))
    return bf16_rne(y)


@pytest.mark.parametrize("perturb", [_truncated, _neighbour_scale, _dropped_k_slice, _shifted_tap],
                         ids=["truncating_rounding", "neighbour_scale", "dropped_k_slice", "shifted_tap"])
def test_perturbed_reference_fails(perturb):
    with pytest.raises(AssertionError):
        assert_ulps(perturb(), _reference(), perturb.__name__)
