"""MobileNetV2 past the 2^31 boundary: the `chunk < B` branch of add_mbv2_block (csrc/api_backbone.hip), which builds the chain of an
InvertedResidual block over runs of images when a tensor of the block would pass conv_igemm's 31-bit element offsets.

  * runs() restates the rule (mbv2_pad, mbv2_ld, the per-image element count, the limit 2^31 - 1) and is pinned against hand values
    without a GPU;
  * single blocks on a ragged 251 x 259 map through Engine.mbv2_block, at the largest batch that is one run (limit), at limit + 1 (a last
    run of ONE image) and at limit + 2: launch counts, the route record of every run, images 0-3 against the restatement
    (tests/mobilenet_ref.py), zero pad channels, every copy of an image bit-identical to the first, the same bits as a 4-image call;
  * one 64-image step of the whole network at 800 x 1333, the smallest full-size batch that splits (features.2: 62 + 2);
  * an image that is too large alone is refused by name before any buffer is allocated.

The batch is four distinct images repeated and is built on the device (the fp32 NCHW input is 1-4 GiB).  Tolerances are the project's:
a block with bf16 intermediates <= 2 ulps at max(|element|, rms), at most 3 % of the elements differing (tests/test_mobilenet_gpu.py);
f32 <= 1e-3 of max(1, the tensor's maximum) (test_parity_modes_always_take_the_chain); B = 4 against B = 64 pyramid within 4e-2 of each
level's scale, logits within 2e-2 relative L2, bf16 pyramid within 5e-2 relative L2 of the fp32 restatement
(tests/test_resnext_gpu.py::test_batch_192_x101_positions_and_batch_sizes).  Measurements: profiles/mobilenet_far_end.txt."""
import os
import time

import pytest
import torch

from oracle import bf16 as OB16
from tests import mobilenet_ref as MR
from tests.test_mobilenet_gpu import CONVS, DW, FUSED, ROUTES, STEM, _assert_route, _block_operands, _engine
from tests.test_resnet_basic_gpu import _assert_ulps

gpu = pytest.mark.gpu
LIMIT = 2 ** 31 - 1  # conv_igemm's largest element offset


# ---- the run rule, restated ----------------------------------------------------------------------------------------------------------
def _pad(c, dtype):
    """mbv2_pad: channels as computed, the K slice of the implicit-GEMM kernels"""
    q = 64 if dtype == "bf16" else 32
    return -(-c // q) * q


def _ld(c, dtype):
    """mbv2_ld: the row pitch, a whole number of conv_igemm's N tiles"""
    p = _pad(c, dtype)
    q = 128 if p >= 128 else 64 if p > 32 else 32
    return -(-p // q) * q


def per_image(shape, H, W, dtype):
    """elements of the largest tensor of one image that a 1x1 launch of the chain addresses"""
    cin, t, cout, stride = shape
    cin_ld, hid_ld, cout_ld = _ld(cin, dtype), _ld(cin * t, dtype), _ld(cout, dtype)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    return max(H * W * max(cin_ld, hid_ld if t != 1 else 0), Ho * Wo * max(hid_ld, cout_ld))


def runs(shape, H, W, B, dtype):
    """images per run of the chain: run, run, ..., remainder"""
    per = per_image(shape, H, W, dtype)
    if per > LIMIT:
        raise ValueError(f"image too large for the MobileNetV2 chain: {per} elements per image")
    run = min(B, LIMIT // per)
    return [run] * (B // run) + ([B % run] if B % run else [])


def test_run_rule_hand_values():
    assert [_pad(c, "bf16") for c in (16, 24, 32, 96, 144, 192, 960)] == [64, 64, 64, 128, 192, 192, 960]
    assert [_pad(c, "f32") for c in (16, 24, 32, 96, 144, 192, 960)] == [32, 32, 32, 96, 160, 192, 960]
    assert [_ld(c, "bf16") for c in (16, 32, 96, 144, 192, 320, 576, 960)] == [64, 64, 128, 256, 256, 384, 640, 1024]
    assert [_ld(c, "f32") for c in (16, 32, 96, 144)] == [32, 32, 128, 256]
    # a 256 x 256 map: per image, run length, the split of the first batch that has a last run of 3
    for dtype, shape, per, run in (("bf16", (16, 6, 24, 2), 2 ** 23, 255),   # hid 96 stored as 128
                                   ("bf16", (24, 6, 24, 1), 2 ** 24, 127),   # hid 144 stored as 256
                                   ("bf16", (32, 1, 16, 1), 2 ** 22, 511),   # t == 1: the expand output does not exist
                                   ("f32", (16, 6, 24, 2), 2 ** 23, 255)):   # hid 96 stored as 128
        assert per_image(shape, 256, 256, dtype) == per
        assert runs(shape, 256, 256, run, dtype) == [run]
        assert runs(shape, 256, 256, run + 1, dtype) == [run, 1]
        assert runs(shape, 256, 256, run + 3, dtype) == [run, 3]
        assert runs(shape, 256, 256, 2 * run + 1, dtype) == [run, run, 1]
    # features.2 of a full-size step: the 800 x 1344 padded input is a 400 x 672 map there
    assert per_image((16, 6, 24, 2), 400, 672, "bf16") == 34406400
    assert runs((16, 6, 24, 2), 400, 672, 62, "bf16") == [62] and runs((16, 6, 24, 2), 400, 672, 64, "bf16") == [62, 2]
    assert runs((16, 6, 24, 2), 400, 672, 192, "bf16") == [62, 62, 62, 6]
    # the ragged map of the block tests
    assert [LIMIT // per_image(s, 251, 259, "bf16") for s in ((16, 6, 24, 2), (24, 6, 24, 1), (32, 1, 16, 1))] == [258, 129, 516]
    assert LIMIT // per_image((16, 6, 24, 2), 251, 259, "f32") == 258
    # one image that passes the limit alone is refused, not built with offsets that wrap
    assert per_image((1, 6, 1, 1), 5800, 5800, "bf16") == 5800 * 5800 * 64 > LIMIT
    with pytest.raises(ValueError, match="image too large for the MobileNetV2 chain: 2152960000 elements per image"):
        runs((1, 6, 1, 1), 5800, 5800, 1, "bf16")


def _whole_network_dw_launches(B, dtype="bf16", fused=frozenset({(32, 1, 16, 1), (24, 6, 24, 1), (32, 6, 32, 1)})):
    """depthwise launches of one 800 x 1344 step: one per run of every block that takes the chain"""
    h, w, n = 400, 672, 0
    for shape in MR.blocks():
        if shape not in fused:
            n += len(runs(shape, h, w, B, dtype))
        h, w = (h - 1) // shape[3] + 1, (w - 1) // shape[3] + 1
    return n


def test_whole_network_run_counts():
    assert _whole_network_dw_launches(62) == 13 and _whole_network_dw_launches(64) == 14
    assert _whole_network_dw_launches(63) == 14  # (features.2: 62 + 1)
    assert _whole_network_dw_launches(192, fused=frozenset()) == 17 + 1 + 3 + 1 + 1  # features.1 - 4 split at 192 images, all chain


# ---- single blocks across the boundary -------------------------------------------------------------------------------------------------
H, W = 251, 259  # ragged: 65 009 positions, no multiple of 8 or 64; stride 2 gives 126 x 130
_REF = {}


def _reference(shape, dtype):
    """operands of four distinct images and the restatement on them, computed once per (shape, dtype)"""
    if (shape, dtype) not in _REF:
        x, ws, scales, shifts, stride = _block_operands(shape, H, W, 4)
        with torch.no_grad():
            want = (MR.block_bf16 if dtype == "bf16" else MR.block)(x, ws, scales, shifts, stride)
        _REF[(shape, dtype)] = (x, ws, scales, shifts, stride, want)
    return _REF[(shape, dtype)]


def _bits(t):
    return t.view(torch.int32)


def _copies_that_differ(y, keep=4):
    """indices k >= keep with y[k] not bit-identical to y[k % keep]; compared on the device"""
    yi, bad = _bits(y), []
    for k in range(keep, y.shape[0], keep):
        n = min(keep, y.shape[0] - k)
        if not torch.equal(yi[k:k + n], yi[:n]):
            bad += [k + i for i in range(n) if not torch.equal(yi[k + i], yi[i])]
    return bad


def _run_block(eng, x4d, B, ws, scales, shifts, stride):
    xb = x4d[torch.arange(B, device=x4d.device) % 4]  # built on the device
    eng.profile_read(), eng.conv_routes()
    y = eng.mbv2_block(xb, ws, scales, shifts, stride, padded=True)
    torch.cuda.synchronize()
    return y, eng.profile_read()["kernels"], eng.conv_routes()


def _assert_chain_launches(kernels, routes, want_runs, t, what):
    n_conv = 1 if t == 1 else 2
    n_1x1 = sum(kernels[k]["launches"] for k in CONVS if k in kernels)
    print(f"{what}: runs {want_runs}, {DW} launches {kernels.get(DW, {}).get('launches')}, 1x1 launches {n_1x1}")
    for i, r in enumerate(want_runs):
        print(f"  run {i} ({r} images): {routes[i * n_conv:(i + 1) * n_conv]}")
    assert set(kernels) <= {DW, *CONVS}, kernels
    assert kernels[DW]["launches"] == len(want_runs), (kernels, want_runs)
    assert n_1x1 == len(want_runs) * n_conv == len(routes), (kernels, routes, want_runs)


CASES = [("bf16", (16, 6, 24, 2), "chain"),    # stride 2, no residual
         ("bf16", (24, 6, 24, 1), "chain"),    # the residual is read from the advanced X
         ("bf16", (32, 1, 16, 1), "chain"),    # t == 1: the depthwise kernel reads the advanced X, h1 unused
         ("f32", (16, 6, 24, 2), "default")]   # fp32 always takes the chain; 8.6 GB of h1


@gpu
@pytest.mark.parametrize("dtype,shape,knob", CASES, ids=lambda v: v if isinstance(v, str) else "c%d_t%d_c%d_s%d" % v)
def test_block_chain_splits_past_the_limit(monkeypatch, dtype, shape, knob):
    t0 = time.perf_counter()
    if knob == "default":
        monkeypatch.delenv("SYLPH_MBV2_FUSED", raising=False)
    else:
        monkeypatch.setenv("SYLPH_MBV2_FUSED", ROUTES[knob])
    x4, ws, scales, shifts, stride, want = _reference(shape, dtype)
    cin, t, cout, _ = shape
    run = LIMIT // per_image(shape, H, W, dtype)
    what = f"block {shape} {H}x{W} {dtype}"
    eng = _engine(dtype, profile=True)
    x4d = x4.cuda()
    y4 = eng.mbv2_block(x4d, ws, scales, shifts, stride, padded=True)
    # the largest batch that is one run, then a last run of one image
    for B in (run, run + 1):
        assert runs(shape, H, W, B, dtype) == ([run] if B == run else [run, 1])
        y, kernels, routes = _run_block(eng, x4d, B, ws, scales, shifts, stride)
        _assert_chain_launches(kernels, routes, runs(shape, H, W, B, dtype), t, f"{what} B{B}")
        bad = _copies_that_differ(y)
        assert not bad, f"{what} B{B}: runs {runs(shape, H, W, B, dtype)}, copies that differ from images 0-3: {bad[:16]} ({len(bad)})"
        assert torch.equal(_bits(y[:4]), _bits(y4)), f"{what} B{B}: images 0-3 differ from the 4-image call"
        del y
    # the smallest batch with a last run of two images: everything
    B = run + 2
    rr = runs(shape, H, W, B, dtype)
    assert rr == [run, 2]
    y, kernels, routes = _run_block(eng, x4d, B, ws, scales, shifts, stride)
    _assert_chain_launches(kernels, routes, rr, t, f"{what} B{B}")
    assert y.shape == (B, eng.mbv2_padded_channels(cout), (H - 1) // stride + 1, (W - 1) // stride + 1)
    assert y.shape[1] > cout and int(torch.count_nonzero(y[:, cout:])) == 0, "pad channels"
    got = y[:4, :cout].cpu()
    if dtype == "bf16":
        _assert_ulps(got, want, f"{what} B{B}", max_ulp=2.0, max_frac=0.03, floor="rms")
    else:
        err, scale = float((got - want).abs().max()), max(1.0, float(want.abs().max()))
        print(f"{what} B{B}: max err {err:.2e}, {err / scale:.2e} of max(1, the tensor's maximum)")
        assert err <= 1e-3 * scale
    bad = _copies_that_differ(y)
    assert not bad, f"{what} B{B}: runs {rr}, copies that differ from images 0-3: {bad[:16]} ({len(bad)})"
    assert not torch.equal(_bits(y[0]), _bits(y[1]))
    assert torch.equal(_bits(y[:4]), _bits(y4)), f"{what} B{B}: images 0-3 differ from the 4-image call"
    eng.close()
    del y, y4, x4d
    torch.cuda.empty_cache()
    print(f"{what}: wall time {time.perf_counter() - t0:.1f} s")


@gpu
def test_block_default_route_is_one_launch_past_the_limit(monkeypatch):
    """(24, 6, 24, 1) with SYLPH_MBV2_FUSED not set: the one-launch kernel with grid.y = B, which indexes with size_t -- no runs"""
    t0 = time.perf_counter()
    monkeypatch.delenv("SYLPH_MBV2_FUSED", raising=False)
    shape, dtype = (24, 6, 24, 1), "bf16"
    x4, ws, scales, shifts, stride, want = _reference(shape, dtype)
    B = LIMIT // per_image(shape, H, W, dtype) + 2
    assert len(runs(shape, H, W, B, dtype)) == 2  # the chain would split here
    eng = _engine(dtype, profile=True)
    x4d = x4.cuda()
    y4 = eng.mbv2_block(x4d, ws, scales, shifts, stride, padded=True)
    y, kernels, routes = _run_block(eng, x4d, B, ws, scales, shifts, stride)
    _assert_route(kernels, "fused", shape[1])
    assert kernels[FUSED]["launches"] == 1 and routes == [], (kernels, routes)
    assert y.shape == (B, 64, H, W) and int(torch.count_nonzero(y[:, 24:])) == 0
    _assert_ulps(y[:4, :24].cpu(), want, f"block {shape} {H}x{W} B{B} default route", max_ulp=2.0, max_frac=0.03, floor="rms")
    bad = _copies_that_differ(y)
    assert not bad, f"copies that differ from images 0-3: {bad[:16]} ({len(bad)})"
    assert not torch.equal(_bits(y[0]), _bits(y[1])) and torch.equal(_bits(y[:4]), _bits(y4))
    eng.close()
    del y, y4, x4d
    torch.cuda.empty_cache()
    print(f"block {shape} default route B{B}: wall time {time.perf_counter() - t0:.1f} s")


@gpu
def test_image_too_large_for_the_chain_is_refused_by_name(monkeypatch):
    """One 5800 x 5800 image of a (1, 6, 1, 1) block has 2.15 G elements in its expand output: refused before a buffer is allocated (the
    input is 135 MB on the device and is never read)."""
    monkeypatch.setenv("SYLPH_MBV2_FUSED", "0")
    shape = (1, 6, 1, 1)
    _, ws, scales, shifts, stride = _block_operands(shape, 2, 2, 1)
    eng = _engine("bf16")
    y = eng.mbv2_block(torch.ones(1, 1, 2, 2), ws, scales, shifts, stride)  # the shape itself runs
    assert y.shape == (1, 1, 2, 2) and bool(torch.isfinite(y).all())
    before = eng.device_bytes()
    x = torch.empty(1, 1, 5800, 5800, device="cuda")
    with pytest.raises(RuntimeError, match=f"image too large for the MobileNetV2 chain: {per_image(shape, 5800, 5800, 'bf16')} elements per image"):
        eng.mbv2_block(x, ws, scales, shifts, stride)
    assert eng.device_bytes() == before
    eng.close()


# ---- one whole-network step that splits --------------------------------------------------------------------------------------------------
def _step(sd, imgs, codes, keep=4):
    """One bf16 query step (the pattern of tests/test_resnext_gpu.py::_step) -> the kernels of the backbone, the pyramid and the head
    outputs of images [0, keep), the detections of those, and what differs between a later group of `keep` images and the first"""
    eng = _engine("bf16", profile=True)
    eng.load_state_dict(sd)
    eng.preprocess(imgs)
    eng.profile_read()
    eng.backbone()
    torch.cuda.synchronize()
    kernels = eng.profile_read()["kernels"]
    differ = []
    pyr = eng.export_pyramid()
    differ += [f"p{l + 3} images {k}.." for l, p in enumerate(pyr) for k in range(keep, len(imgs), keep) if not torch.equal(_bits(p[:keep]), _bits(p[k:k + keep]))]
    pyr = [p[:keep].clone() for p in pyr]
    eng.head(codes["cls_conv"], codes["cls_bias"])
    outs = [torch.cat([t.flatten(1) for t in ts], 1) for ts in eng.export_head()]
    differ += [f"head output {i} images {k}.." for i, o in enumerate(outs) for k in range(keep, len(imgs), keep) if not torch.equal(_bits(o[:keep]), _bits(o[k:k + keep]))]
    outs = [o[:keep].clone() for o in outs]
    dets = [{k: v.cpu() for k, v in d.items() if torch.is_tensor(v)} for d in eng.decode()]
    differ += [f"detections of image {i}: {k}" for i in range(keep, len(imgs)) for k in dets[i] if not torch.equal(dets[i][k], dets[i % keep][k])]
    eng.close()
    del eng
    torch.cuda.empty_cache()
    return kernels, pyr, outs, dets[:keep], differ


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _network_operands():
    from sylph_amd import synthetic as Wt
    sd = Wt.mobilenet_backbone_state_dict(0)
    sd.update(Wt.head_state_dict(1, num_classes=60))
    return sd, Wt.synthetic_images(4, 800, 1333, seed=3), Wt.synthetic_codes(5, seed=4, scale=3.0)


@gpu
def test_batch_64_full_size_step_splits_features_2(monkeypatch):
    """64 images of 800 x 1333 (four images x 16), default knobs: the smallest full-size batch at which a block of the network is built
    over runs (features.2, the chain on a 400 x 672 map: 62 + 2)."""
    from oracle import backbone as OB
    t0 = time.perf_counter()
    monkeypatch.delenv("SYLPH_MBV2_FUSED", raising=False)
    try:
        torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    except AttributeError:
        pass
    sd, four, codes = _network_operands()
    k64, p64, o64, d64, differ = _step(sd, [four[i % 4] for i in range(64)], codes)
    print({k: v["launches"] for k, v in k64.items()})
    assert k64[DW]["launches"] == _whole_network_dw_launches(64) == 14 and k64[FUSED]["launches"] == 4 and k64[STEM]["launches"] == 1, k64
    assert not differ, f"copies in the 64-image step that differ from images 0-3: {differ[:8]}"
    assert all(d["scores"].numel() > 0 for d in d64)
    k4, p4, o4, _, _ = _step(sd, four, codes)
    assert k4[DW]["launches"] == 13 and k4[FUSED]["launches"] == 4, k4
    for l, (a, b) in enumerate(zip(p4, p64)):
        err = float((a - b).abs().max()) / float(b.abs().max())
        print(f"p{l + 3}: B = 4 vs B = 64 max err {err:.2e} of the level's scale (bit-identical: {torch.equal(a, b)})")
        assert err <= 4e-2
    rel = _rel(o4[0], o64[0])
    print(f"logits: B = 4 vs B = 64 relative L2 {rel:.2e}")
    assert rel <= 2e-2
    x, _ = OB.preprocess(four[:1])
    with torch.no_grad():
        pyr_ref = MR.mobilenet_backbone_fpn(x, sd)
    for l, (a, b) in enumerate(zip(p64, pyr_ref)):
        rel = _rel(a[0].cpu(), b[0])
        print(f"p{l + 3}: bf16 B = 64 vs fp32 restatement relative L2 {rel:.2e}")
        assert rel <= 5e-2
    print(f"64-image step: wall time {time.perf_counter() - t0:.1f} s")
