"""3x3 class codes (MODEL.META_LEARN.CODE_GENERATOR.CLS_LAYER = ["", "", 3]) on the GPU.

Query head: `F.conv2d(cls_tower, W[N, 256, 3, 3], bias, padding = 1)` on every level -- a cross-correlation whose zero padding applies
to the NORMALISED tower output relu(GN(x)), not to x (relu(b) of a GroupNorm coefficient is not zero).  Two routes:
  generic  the deferred GroupNorm apply, if any, then add_conv with pad 1 on the packed codes: what sylph_fcos_head_pretrained builds for
           a 3x3 cls_logits.  Every dtype and class count, and the default
  fused    gn_cond3x3_kernel (csrc/head_fused.hip): bf16, GroupNorm towers, N <= 32 -- last cls GroupNorm + ReLU + the 3x3 conv in one
           pass; taken only with SYLPH_GN_COND3X3=1 (read per head call) while it does not beat the generic route
The kernel cases run random bf16-representable features through Engine.import_pyramid at padded (96, 160) (levels 12x20, 6x10, 3x5,
2x3, 1x2: 32-position groups that straddle map rows, ragged last groups, levels smaller than one group, a level with no row above or
below), all images distinct.  Every kernel case asserts, from the exported coefficient tables, that relu(b) > 0 somewhere, and, from
the kernel profile, which route ran.

References and bounds (none of them new):
  * logits against F.conv2d(xn, W, padding = 1) + bias on the operands the graph stored (export_tower + oracle.bf16.gn_apply): fused
    kernel: the project's bound for fp32 head outputs, _assert_f32 (the 3x3 prediction convs meet it at the same K = 2 304); generic
    route: the bounds tests/test_hip_parity.py applies to g1_head_decode.npz in each dtype (fp32 / f32s 1e-3, bf16 4e-2 of the scale);
  * the reference's own outputs (g10_spatial_codes.npz) through the C ABI with the bounds of the g3 / g1 GPU tests."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import spatial_codes_ref as R
from test_bf16_pinned_gpu import _assert_f32
from test_head_sweeps_gpu import HW, LEVELS, _new, _normalised, _pin, _premises, _pyramid, _where_sweep
from test_hip_parity import _cfg, _feats
from test_mixed_episodes_gpu import FIELDS, _code, _kernels

pytestmark = pytest.mark.gpu

K3 = "MODEL.META_LEARN.CODE_GENERATOR.CLS_LAYER"
FUSED = "gn_cond3x3_kernel"
KNOB = "SYLPH_GN_COND3X3"  # read at every head call
# N -> (seed, per-tap scale); 9: the adversarial one-tap codes
CODES = {1: (71, 1.2), 5: (72, 1.0), 8: (73, 1.0), 32: (74, 0.8), 33: (75, 0.8)}


def _cfg3(**over):
    return _cfg(**{K3: ["", "", 3], **over})


def _codes(n):
    c = R.one_tap_codes(seed=79, scale=2.5) if n == 9 else R.spatial_codes(n, *CODES[n])
    return {k: v.cuda() for k, v in c.items()}


def _want(xn, c, round_w):
    """the reference of every kernel case: F.conv2d(xn, W, padding = 1) + bias per level (bf16 engines pack the codes to bf16)"""
    from oracle import bf16 as OB16
    w = c["cls_conv"].cpu()
    return [R.cond_conv(x, OB16.r(w) if round_w else w, None) + c["cls_bias"].cpu().view(1, -1, 1, 1) for x in xn]


def _relu_b_positive(coefs):
    """the premise that makes "pad before the norm" fail: some GroupNorm coefficient b of the last cls layer is > 0"""
    return any(bool((cf[:, :, 1] > 0).any()) for cf in coefs)


@pytest.fixture(scope="module")
def sd():
    from sylph_amd import synthetic as Wt
    return Wt.head_state_dict(seed=1, num_classes=60)


@pytest.fixture(scope="module")
def pyr3():
    return _pyramid(3, LEVELS, seed=21)


@pytest.fixture(scope="module")
def fused3(pyr3, sd):
    """One bf16 engine over the 3-image batch; the normalised last cls layer (it does not depend on the codes) and its coefficient
    tables, taken after a FUSED head (which leaves the stored tower output un-normalised)"""
    eng = _new(_cfg3(), sd, pyr3, HW)
    assert eng.level_shapes(*HW) == LEVELS and eng.code_ksize == 3
    c = _codes(5)
    os.environ[KNOB] = "1"
    try:
        eng.head(c["cls_conv"], c["cls_bias"])
    finally:
        del os.environ[KNOB]
    coefs = [cf.cpu() for cf in eng.export_tower(0, 3)[1]]
    case = {"eng": eng, "xn": _normalised(eng, 0), "coefs": coefs, "pred": [[t.clone() for t in lv] for lv in eng.export_head()[1:]]}
    yield case
    eng.close()


# ------------------------------------------------------------------------------------------------ 5: the fused kernel
@pytest.mark.parametrize("n", [1, 5, 8, 9, 32])
def test_fused_kernel_matches_conv_on_stored_operands(fused3, n, monkeypatch):
    monkeypatch.setenv(KNOB, "1")
    eng, c = fused3["eng"], _codes(n)
    assert _relu_b_positive(fused3["coefs"])
    k = _kernels(eng, lambda: eng.head(c["cls_conv"], c["cls_bias"]))
    assert k.get(FUSED) == 1 and "gn_logits_kernel" not in k and "logits_scan_kernel" not in k, k
    lo, rg, ct, io = eng.export_head()
    want = _want(fused3["xn"], c, round_w=True)
    for l in range(5):
        assert tuple(lo[l].shape) == (3, n) + LEVELS[l]
        _pin(lo[l], want[l], f"N={n} logits level {l}", l, lambda i, lv, row: f"group {row // 32} of its level")
        # padding BEFORE the norm would add relu(b) at the border taps: far outside the bound where the map has a border
        for got, ref in zip((rg[l], ct[l], io[l]), (p[l] for p in fused3["pred"])):
            assert torch.equal(got, ref)


def test_fused_kernel_box_branch_equals_1x1_head(fused3, pyr3, sd):
    """box regression, centerness and IoU do not see the codes: bit for bit those of a k = 1 engine on the same batch"""
    eng1 = _new(_cfg(), sd, pyr3, HW)
    c = _code("n5")
    eng1.head(c["cls_conv"], c["cls_bias"])
    for got, ref in zip(eng1.export_head()[1:], fused3["pred"]):
        for l in range(5):
            assert torch.equal(got[l], ref[l])
    eng1.close()


def test_default_route_is_the_generic_one(fused3):
    """without the knob bf16 N <= 32 takes the apply + conv_igemm launches, and gives the fused kernel's logits to the fused bound"""
    eng, c = fused3["eng"], _codes(5)
    assert KNOB not in os.environ
    k = _kernels(eng, lambda: eng.head(c["cls_conv"], c["cls_bias"]))
    assert FUSED not in k and k.get("gn_apply_partials_kernel") == 1 and k.get("conv_igemm_kernel", 0) >= 1, k
    want = _want(fused3["xn"], c, round_w=True)
    for l, t in enumerate(eng.export_head()[0]):
        _assert_f32(t, want[l], f"default route: logits level {l}")


def test_pad_before_norm_would_be_seen(fused3, monkeypatch):
    """the reference of the kernel cases tells the two paddings apart on this batch by far more than the bound"""
    monkeypatch.setenv(KNOB, "1")
    from oracle import bf16 as OB16
    eng, c = fused3["eng"], _codes(5)
    eng.head(c["cls_conv"], c["cls_bias"])  # a fused head leaves the stored tower output un-normalised
    ys, cfs = eng.export_tower(0, 3)
    y, cf = ys[0].cpu(), cfs[0].cpu()
    wrong = OB16.gn_apply(F.pad(y, (1, 1, 1, 1)), cf)  # zero padding of x: relu(b) at the border
    got = F.conv2d(wrong, OB16.r(c["cls_conv"].cpu())) + c["cls_bias"].cpu().view(1, -1, 1, 1)
    want = _want(fused3["xn"], c, True)[0]
    assert float((got - want).abs().max()) > 100 * 1e-4 * max(1.0, float(want.abs().max()))


# ------------------------------------------------------------------------------------------------ 6: sweeps of the capped grid
def test_fused_kernel_two_sweeps(sd, monkeypatch):
    """B = 352: 2 112 tiles, the kernel launches min(n_tiles, CAP) blocks and blocks 0-63 take a second tile (another image, another
    level: the coefficient table is reloaded, the codes stay in registers)"""
    monkeypatch.setenv(KNOB, "1")
    feats = _pyramid(352, LEVELS, seed=22)
    eng = _new(_cfg3(), sd, feats, HW)
    _premises(eng, 352, HW, LEVELS, n_tiles=2112, sweeps=2)
    c = _codes(5)
    k = _kernels(eng, lambda: eng.head(c["cls_conv"], c["cls_bias"]))
    assert k.get(FUSED) == 1, k
    ys, cfs = eng.export_tower(0, 3)
    assert _relu_b_positive([cf.cpu() for cf in cfs])
    want = _want(_normalised(eng, 0), c, True)
    lo = eng.export_head()[0]
    for l in range(5):
        _pin(lo[l], want[l], f"two sweeps: logits level {l}", l, _where_sweep(LEVELS))
    eng.close()


# ------------------------------------------------------------------------------------------------ 7: position in the batch
def test_logits_do_not_depend_on_the_position_in_the_batch(pyr3, sd, monkeypatch):
    """image 0 alone, and as image 2 of B = 3: torch.equal logits on every level (a tap never reads a neighbour's rows)"""
    monkeypatch.setenv(KNOB, "1")
    c = _codes(5)
    alone = _new(_cfg3(), sd, [f[:1] for f in pyr3], HW)
    alone.head(c["cls_conv"], c["cls_bias"])
    la, ta = alone.export_head()[0], alone.export_tower(0, 3)[0]
    order = [1, 2, 0]
    three = _new(_cfg3(), sd, [f[order] for f in pyr3], HW)
    k = _kernels(three, lambda: three.head(c["cls_conv"], c["cls_bias"]))
    assert k.get(FUSED) == 1, k
    lt, tt = three.export_head()[0], three.export_tower(0, 3)[0]
    for l in range(5):
        assert torch.equal(ta[l][0], tt[l][2]), f"premise: the cls tower output of the image differs with the batch (level {l})"
        assert torch.equal(la[l][0], lt[l][2]), f"level {l}: max |diff| {float((la[l][0] - lt[l][2]).abs().max())}"
        assert not torch.equal(lt[l][0], lt[l][2])  # the images are distinct
    alone.close()
    three.close()


# ------------------------------------------------------------------------------------------------ 8: the generic route
def _generic_case(eng, c, warm):
    """head with `c` under the profile, after a head with other codes has built the plan: the routes recorded are those of the ONE conv
    the call added"""
    eng.head(warm["cls_conv"], warm["cls_bias"])
    eng.profile_enable(True)
    eng.conv_routes()
    eng.profile_enable(False)
    k = _kernels(eng, lambda: eng.head(c["cls_conv"], c["cls_bias"]))
    routes = eng.conv_routes()
    assert FUSED not in k and k.get("conv_igemm_kernel", 0) >= 1 and "gn_logits_kernel" not in k and "logits_scan_kernel" not in k, k
    assert len(routes) == 1 and routes[0].split()[0] in ("igemm", "igemm_halo"), routes
    return k


def test_generic_route_bf16_many_way(fused3, monkeypatch):
    """N = 33 > 32: the deferred GroupNorm apply, then conv_igemm on the packed 3x3 codes (bf16 bound of the g1 head test: 4e-2)"""
    monkeypatch.setenv(KNOB, "1")  # (N = 33 takes the generic route whatever the knob says; the fused head afterwards needs it)
    eng, c = fused3["eng"], _codes(33)
    assert _relu_b_positive(fused3["coefs"])
    _generic_case(eng, c, _codes(1))
    lo = eng.export_head()[0]
    want = _want(fused3["xn"], c, round_w=True)
    for l in range(5):
        err = float((lo[l].cpu() - want[l]).abs().max()) / max(1.0, float(want[l].abs().max()))
        print(f"bf16 N=33 level {l}: relative deviation {err:.3e}")
        assert err < 4e-2, (l, err)
    # the apply ran in place: a fused head afterwards starts from fresh tower outputs and still meets its bound
    c5 = _codes(5)
    k = _kernels(eng, lambda: eng.head(c5["cls_conv"], c5["cls_bias"]))
    assert k.get(FUSED) == 1, k
    _assert_f32(eng.export_head()[0][0], _want(fused3["xn"], c5, True)[0], "fused head after a generic one, level 0")


@pytest.mark.parametrize("dtype", ["f32", "f32s"])
def test_generic_route_fp32_storage(fused3, pyr3, sd, dtype):
    """fp32 / f32s, N = 5: the head ops apply every GroupNorm themselves; 1e-3 as for g1 in these modes.  The stored last layer is the
    normalised tensor itself and there is no coefficient table to export: the relu(b) > 0 premise is formed from this engine's own
    stored input of the last layer (layer 2's output) -- its conv and GroupNorm statistics on the host, oracle.bf16.gn_coef."""
    from oracle import bf16 as OB16
    from sylph_amd.engine import Engine
    eng = Engine(_cfg3(), dtype=dtype)
    eng.load_state_dict(sd)
    eng.set_debug_taps(True)
    eng.import_pyramid(pyr3, HW)
    c = _codes(5)
    _generic_case(eng, c, _codes(1))
    xn = [y.cpu() for y in eng.export_tower(0, 3, with_coef=False)[0]]
    assert all(float(x.min()) >= 0.0 for x in xn)  # applied in place: relu(GN(.))
    p = "proposal_generator.fcos_head.cls_tower"
    coefs = [OB16.gn_coef(F.conv2d(x2.cpu(), sd[f"{p}.9.weight"], sd[f"{p}.9.bias"], padding=1), sd[f"{p}.10.weight"], sd[f"{p}.10.bias"])
             for x2 in eng.export_tower(0, 2, with_coef=False)[0]]
    assert _relu_b_positive(coefs)
    lo = eng.export_head()[0]
    want = _want(xn, c, round_w=False)
    for l in range(5):
        np.testing.assert_allclose(lo[l].cpu().numpy(), want[l].numpy(), atol=1e-3, rtol=1e-3)
    eng.close()


def test_generic_route_without_tower_norm(pyr3):
    """MODEL.FCOS.NORM "none", bf16: no coefficient table, so the conv route on the stored (ReLU) tower output"""
    from oracle import bf16 as OB16
    from sylph_amd import synthetic as Wt
    from sylph_amd.engine import Engine
    eng = Engine(_cfg3(**{"MODEL.FCOS.NORM": "none"}), dtype="bf16")
    eng.load_state_dict(Wt.head_state_dict(seed=1, num_classes=60, norm="none"))
    eng.set_debug_taps(True)
    eng.import_pyramid(pyr3, HW)
    c = _codes(5)
    _generic_case(eng, c, _codes(1))
    xn = [y.cpu() for y in eng.export_tower(0, 3, with_coef=False)[0]]
    lo = eng.export_head()[0]
    want = _want(xn, c, round_w=True)
    for l in range(5):
        _assert_f32(lo[l], want[l], f"NORM none: logits level {l}")  # exact bf16 operands, fp32 sums
    eng.close()


# ------------------------------------------------------------------------------------------------ 9: the reference's outputs through the C ABI
@pytest.fixture(scope="module")
def g10(golden_dir):
    return np.load(os.path.join(golden_dir, "g10_spatial_codes.npz"))


@pytest.fixture(scope="module")
def g3(golden_dir):
    return np.load(os.path.join(golden_dir, "g3_codegen.npz"))


@pytest.fixture(scope="module")
def g1(golden_dir):
    return np.load(os.path.join(golden_dir, "g1_head_decode.npz"))


def _support_engine(tag, dtype):
    from sylph_amd import synthetic as Wt
    from sylph_amd.engine import Engine
    over = {}
    if tag == "ws":
        over = {"MODEL.META_LEARN.CODE_GENERATOR.WEIGHT_LAYER": ["", "", 1], "MODEL.META_LEARN.CODE_GENERATOR.SCALE_LAYER": ["", "", 1]}
    if tag == "l2":
        over = {"MODEL.META_LEARN.CODE_GENERATOR.BIAS_L2_NORM": True}
    eng = Engine(_cfg3(**over), dtype=dtype)
    eng.load_state_dict(Wt.codegen_state_dict(seed=2, weight_scale_layers=tag == "ws"))
    return eng


@pytest.mark.parametrize("dtype", ["f32", "f32s", "bf16"])
@pytest.mark.parametrize("tag", ["sup", "ws", "l2"])
def test_support_codes_match_reference_golden(g10, g3, tag, dtype):
    """raw codes: fp32 / f32s 1e-3 (g3's bound), bf16 cosine > 0.99 and bias within 5e-2 (the bf16 support bound of test_hip_parity);
    normalisation of the reference's raw codes: fp32 arithmetic in every mode, g3's 1e-5 / 1e-4"""
    eng = _support_engine(tag, dtype)
    assert eng.code_len == 2305
    shots = (1, 2, 5) if tag == "sup" else (2, 5)
    for S in shots:
        eng.import_pyramid(_feats(g3, f"s{S}_feat"), (192, 256))
        code = eng.codegen(torch.from_numpy(g3[f"s{S}_boxes"])).cpu()
        assert tuple(code.shape) == (2305,)
        want_w, want_b = g10[f"{tag}_s{S}_cls_conv"].reshape(-1), float(g10[f"{tag}_s{S}_cls_bias"].reshape(-1)[0])
        if dtype == "bf16":
            cos = F.cosine_similarity(code[:2304], torch.from_numpy(want_w), dim=0).item()
            print(f"bf16 {tag} S={S}: cosine {cos:.5f}, bias {code[2304].item():.4f} vs {want_b:.4f}")
            assert cos > 0.99 and abs(code[2304].item() - want_b) < 5e-2
        else:
            np.testing.assert_allclose(code[:2304].numpy(), want_w, atol=1e-3, rtol=1e-3)
            np.testing.assert_allclose(code[2304].item(), want_b, atol=1e-3, rtol=1e-3)
        if tag == "ws":
            wn = eng.codegen_weight_norm(1).cpu()
            tol = 5e-2 if dtype == "bf16" else 1e-3
            assert abs(wn.item() - float(g10[f"ws_s{S}_cls_weight_norm"].reshape(-1)[0])) < tol
    rows = torch.stack([torch.cat([torch.from_numpy(g10[f"{tag}_s{S}_cls_conv"]).reshape(-1), torch.from_numpy(g10[f"{tag}_s{S}_cls_bias"]).reshape(-1)])
                        for S in shots])
    wn = torch.cat([torch.from_numpy(g10[f"ws_s{S}_cls_weight_norm"]).reshape(-1) for S in shots]) if tag == "ws" else None
    out = eng.normalize_codes(rows.cuda().contiguous(), wn).cpu().numpy()
    for i, S in enumerate(shots):
        np.testing.assert_allclose(out[i, :2304], g10[f"{tag}_s{S}_norm_cls_conv"].reshape(-1), atol=1e-5, rtol=1e-4)
        np.testing.assert_allclose(out[i, 2304], g10[f"{tag}_s{S}_norm_cls_bias"].reshape(-1)[0], atol=1e-5, rtol=1e-4)
    eng.close()


@pytest.mark.parametrize("dtype", ["f32", "f32s", "bf16"])
@pytest.mark.parametrize("tag", ["sup", "ws"])
def test_roi_list_codes_equal_class_codes(tag, dtype):
    """codegen_tail_kernel at k = 3, through both entry points: a ROI list is bit-identical to codegen_classes on the batch that repeats
    each image per instance"""
    from test_support_bf16_pinned_gpu import _box_sets, _pyramid as _sup_pyramid
    from test_support_rois_gpu import H as SH, W as SW, _dup, _roi_images
    B, Rn, shots = 4, 12, 3
    feats = _sup_pyramid(B, SH, SW, seed=31)
    roi_image = _roi_images(Rn, B, unused=1, heavy=2, seed=Rn)
    boxes = _box_sets(Rn, SH, SW, seed=100 + Rn)[0]
    eng = _support_engine(tag, dtype)
    eng.import_pyramid(feats, (SH, SW))
    codes = eng.codegen_rois(boxes, roi_image, [shots] * (Rn // shots)).clone()
    wn = eng.codegen_weight_norm(Rn // shots).clone() if tag == "ws" else None
    assert tuple(codes.shape) == (Rn // shots, 2305)
    eng.import_pyramid(_dup(feats, roi_image), (SH, SW))
    want = eng.codegen_classes(boxes, shots)
    assert torch.equal(codes, want), f"max |diff| {float((codes - want).abs().max())}"
    assert float(codes[:, :2304].abs().max()) > 0 and not torch.equal(codes[0], codes[1])
    # the nine taps of a channel differ (a code that repeated the global mean nine times would pass everything above)
    assert float((codes[:, :2304].view(-1, 256, 9).amax(2) - codes[:, :2304].view(-1, 256, 9).amin(2)).abs().max()) > 0
    if wn is not None:
        assert torch.equal(wn, eng.codegen_weight_norm(Rn // shots))
    eng.close()


def _head_engine(dtype, g10, g1):
    from sylph_amd import synthetic as Wt
    from sylph_amd.engine import Engine
    eng = Engine(_cfg3(), dtype=dtype)
    eng.load_state_dict(Wt.head_state_dict(seed=1, num_classes=60))
    sizes = [tuple(int(v) for v in s) for s in g10["image_sizes"]]
    eng.import_pyramid(_feats(g1), (128, 160), sizes)
    return eng, sizes


@pytest.mark.parametrize("dtype", ["f32", "f32s", "bf16"])
@pytest.mark.parametrize("tag", ["n1", "n5", "n20", "tap9"])
def test_head_logits_match_reference_golden(g10, g1, tag, dtype):
    """fp32 / f32s: 1e-3 (test_head_matches_reference_golden); bf16: 4e-2 of the scale (test_head_bf16_close_to_reference_golden)"""
    eng, _ = _head_engine(dtype, g10, g1)
    eng.head(torch.from_numpy(g10[f"{tag}_cls_conv"]), torch.from_numpy(g10[f"{tag}_cls_bias"]))
    lo, rg, ct, io = eng.export_head()
    worst = 0.0
    for l in range(5):
        pairs = ((lo[l], g10[f"{tag}_logits{l}"]), (rg[l], g10[f"reg{l}"]), (ct[l], g10[f"ctr{l}"]), (io[l], g10[f"iou{l}"]))
        for got, want in pairs:
            if dtype == "bf16":
                worst = max(worst, float(np.abs(got.cpu().numpy() - want).max() / max(1.0, np.abs(want).max())))
            else:
                np.testing.assert_allclose(got.cpu().numpy(), want, atol=1e-3, rtol=1e-3)
    if dtype == "bf16":
        print(f"bf16 head vs reference golden ({tag}): worst relative deviation {worst:.4f}")
        assert worst < 4e-2, worst
    eng.close()


def _triples(d):
    lv, loc, cl = (np.asarray(d[k].cpu() if torch.is_tensor(d[k]) else d[k]) for k in ("fpn_levels", "locations", "pred_classes"))
    return set(zip(lv.tolist(), map(tuple, loc.tolist()), cl.tolist()))


@pytest.mark.parametrize("dtype", ["f32", "f32s"])
@pytest.mark.parametrize("tag", ["n5", "tap9"])
def test_detections_match_reference_golden(g10, g1, tag, dtype):
    """the reference's predict_proposals (+ the oracle's detector_postprocess).  fp32: identical (level, location, class) triples in
    order, scores / boxes 1e-3 (test_decode_matches_reference_golden); f32s (2^-17 per product): near-tied scores may trade places and
    one candidate at the post-NMS cut may differ -- the set treatment of test_unequal_tower_depths_match_reference_golden"""
    from oracle.decode import detector_postprocess
    eng, sizes = _head_engine(dtype, g10, g1)
    eng.head(torch.from_numpy(g10[f"{tag}_cls_conv"]), torch.from_numpy(g10[f"{tag}_cls_bias"]))
    dets = eng.decode()
    for i, d in enumerate(dets):
        pre = f"{tag}_img{i}"
        ref = {k: torch.from_numpy(g10[f"{pre}_{k}"]) for k in ("pred_boxes", "scores", "pred_classes", "fpn_levels", "locations")}
        ref = detector_postprocess(ref, sizes[i], sizes[i][0], sizes[i][1])
        if dtype == "f32":
            assert d["scores"].numel() == ref["scores"].numel() > 0
            np.testing.assert_array_equal(d["pred_classes"].cpu().numpy(), ref["pred_classes"].numpy())
            np.testing.assert_array_equal(d["fpn_levels"].cpu().numpy(), ref["fpn_levels"].numpy())
            np.testing.assert_array_equal(d["locations"].cpu().numpy(), ref["locations"].numpy())
            np.testing.assert_allclose(d["scores"].cpu().numpy(), ref["scores"].numpy(), atol=1e-3)
            np.testing.assert_allclose(d["pred_boxes"].cpu().numpy(), ref["pred_boxes"].numpy(), atol=1e-3, rtol=1e-4)
        else:
            gk, rk = _triples(d), _triples(ref)
            assert len(gk ^ rk) <= 2 and abs(len(gk) - len(rk)) <= 1 and len(rk) > 0, (len(gk), len(rk), len(gk ^ rk))
    eng.close()


@pytest.mark.parametrize("tag", ["n5", "tap9"])
def test_bf16_detections_equal_oracle_decode_of_own_logits(g10, g1, tag, monkeypatch):
    """the bf16 step (fused kernel -> decode): its detections are oracle.decode's on the head outputs it exported"""
    monkeypatch.setenv(KNOB, "1")
    from oracle import decode as D
    eng, sizes = _head_engine("bf16", g10, g1)
    w, b = torch.from_numpy(g10[f"{tag}_cls_conv"]), torch.from_numpy(g10[f"{tag}_cls_bias"])
    k = _kernels(eng, lambda: eng.head(w, b))
    assert k.get(FUSED) == 1, k
    dets = eng.decode()
    lo, rg, ct, io = ([t.cpu() for t in lv] for lv in eng.export_head())
    props = D.predict_proposals(lo, rg, ct, io, pre_nms_thresh=0.05)
    for i, d in enumerate(dets):
        ref = D.detector_postprocess(props[i], sizes[i], sizes[i][0], sizes[i][1])
        assert d["scores"].numel() == ref["scores"].numel() > 0
        np.testing.assert_array_equal(d["pred_classes"].cpu().numpy(), ref["pred_classes"].numpy())
        np.testing.assert_array_equal(d["fpn_levels"].cpu().numpy(), ref["fpn_levels"].numpy())
        np.testing.assert_array_equal(d["locations"].cpu().numpy(), ref["locations"].numpy())
        np.testing.assert_allclose(d["scores"].cpu().numpy(), ref["scores"].numpy(), atol=1e-3)
        np.testing.assert_allclose(d["pred_boxes"].cpu().numpy(), ref["pred_boxes"].numpy(), atol=1e-3, rtol=1e-4)
    eng.close()


# ------------------------------------------------------------------------------------------------ 10: the API
def _model_cfg(k):
    from sylph_amd.runner import MetaFCOSRunner, create_cfg
    r = MetaFCOSRunner()
    return r, create_cfg(r.get_default_cfg(), "sylph://COCO-Detection/Meta-FCOS/Meta-FCOS-finetune.yaml", [K3, ["", "", k]])


@pytest.fixture(scope="module")
def full_sd():
    from sylph_amd import synthetic as Wt
    return Wt.synthetic_state_dict(0, depth=50)


@pytest.fixture(scope="module")
def model3(full_sd):
    runner, cfg = _model_cfg(3)
    m = runner.build_model(cfg, dtype="bf16")
    m.load_state_dict(full_sd)
    return m.eval()


def test_model_run_types_carry_3x3_codes(model3):
    from sylph_amd.data import SyntheticQueryLoader, SyntheticSupportSetLoader
    from sylph_amd.evaluation import (format_class_codes_shared, inference_normalization, inference_on_dataset_with_class_codes,
                                      inference_on_support_set_dataset)
    from sylph_amd.structures import Boxes, Instances
    item = next(iter(SyntheticSupportSetLoader(1, 2, 128, 160, seed=3)))
    code = model3(item, run_type="meta_learn_test_support")
    assert tuple(code["cls_conv"].shape) == (1, 256, 3, 3) and tuple(code["cls_bias"].shape) == (1, 1, 1, 1)
    # the ROI-list entry
    recs = item[0]["support_set"]
    segs = [{"image_index": torch.tensor([0, 1]), "boxes": torch.cat([r["instances"].gt_boxes.tensor for r in recs])}]
    roi = model3.forward_class_codes_rois(recs, segs)
    assert len(roi) == 1 and tuple(roi[0]["cls_conv"].shape) == (1, 256, 3, 3) and torch.equal(roi[0]["cls_conv"], code["cls_conv"])
    # loop A -> normalise -> format -> loop B on one rank
    sub = inference_on_support_set_dataset(model3, SyntheticSupportSetLoader(3, 2, 128, 160, seed=3))
    assert all(tuple(c["class_code"]["cls_conv"].shape) == (1, 256, 3, 3) for c in sub)
    sub = inference_normalization(model3, sub)
    for c in sub:
        assert tuple(c["class_code"]["cls_conv"].shape) == (1, 256, 3, 3) and tuple(c["class_code"]["cls_bias"].shape) == (1,)
        taps = c["class_code"]["cls_conv"].norm(dim=1).reshape(-1)
        assert float((taps - taps[0]).abs().max()) < 1e-4  # every tap's L2 norm over the channels is conv_scale
    codes = format_class_codes_shared(sub, model3.device)
    assert tuple(codes["cls_conv"].shape) == (3, 256, 3, 3) and tuple(codes["cls_bias"].shape) == (3,)
    boosted = {"cls_conv": codes["cls_conv"] * 8.0, "cls_bias": codes["cls_bias"]}
    qry = SyntheticQueryLoader(2, 120, 152, batch_size=2, seed=4)
    batch = next(iter(qry))
    out = model3(batch, class_code=boosted, run_type="meta_learn_test_instance")
    assert len(out) == 2 and all(isinstance(o["instances"], Instances) and o["instances"].image_size == (120, 152) for o in out)
    assert sum(len(o["instances"]) for o in out) > 0 and all(int(o["instances"].pred_classes.max()) < 3 for o in out if len(o["instances"]))

    class _Count:
        def reset(self):
            self.n = 0

        def process(self, inputs, outputs):
            self.n += len(outputs)

        def evaluate(self):
            return {"n": self.n}
    assert inference_on_dataset_with_class_codes(model3, qry, _Count(), boosted) == {"n": 2}
    # a list of dicts is the mixed-episode head: refused by name
    with pytest.raises(NotImplementedError, match="CLS_LAYER"):
        model3(batch, class_code=[boosted, boosted], run_type="meta_learn_test_instance")


def test_engine_rejects_the_other_code_size(model3, pyr3, sd):
    eng3 = model3.engine
    with pytest.raises(ValueError, match=r"1x1.*3x3"):
        eng3.head(torch.zeros(2, 256, 1, 1), torch.zeros(2))
    with pytest.raises(NotImplementedError, match="CLS_LAYER"):
        eng3.head_episodes([(torch.zeros(2, 256, 3, 3), torch.zeros(2))], [0])
    with pytest.raises(ValueError, match="CLS_LAYER"):
        eng3.normalize_codes(torch.zeros(1, 257, device="cuda"))
    eng1 = _new(_cfg(), sd, pyr3, HW)
    with pytest.raises(ValueError, match=r"3x3.*1x1"):
        eng1.head(torch.zeros(2, 256, 3, 3), torch.zeros(2))
    eng1.close()


def test_owd_on_a_3x3_engine(pyr3, sd):
    """MODEL.PROPOSAL_GENERATOR.OWD does not read the codes (one all-ones class: a zero code with bias 40): on a k = 3 engine the
    logits are the constant 40 and the detections are those of the k = 1 engine"""
    dets = []
    for cfg, w in ((_cfg(**{"MODEL.PROPOSAL_GENERATOR.OWD": True}), torch.zeros(3, 256, 1, 1)),
                   (_cfg3(**{"MODEL.PROPOSAL_GENERATOR.OWD": True}), torch.zeros(3, 256, 3, 3))):
        eng = _new(cfg, sd, pyr3, HW)
        eng.head(w, torch.zeros(3))
        lo = eng.export_head()[0]
        assert all(tuple(t.shape[:2]) == (3, 1) and bool((t == 40.0).all()) for t in lo)
        dets.append(eng.decode())
        eng.close()
    assert sum(d["scores"].numel() for d in dets[0]) > 0
    for a, b in zip(*dets):
        for f in FIELDS:
            assert torch.equal(a[f], b[f]), f


def test_c_abi_refuses_episodes_and_packed_rows_with_3x3_codes(pyr3, sd):
    import ctypes
    eng = _new(_cfg3(), sd, pyr3, HW)
    w, b = torch.zeros(2, 2304, device="cuda"), torch.zeros(2, device="cuda")
    rc = eng.L.sylph_fcos_head_episodes(eng._ctx, 1, ctypes.c_void_p(w.data_ptr()), ctypes.c_void_p(b.data_ptr()), (ctypes.c_int * 1)(2),
                                        (ctypes.c_int * 3)(0, 0, 0))
    assert rc != 0 and b"CLS_LAYER" in eng.L.sylph_last_error()
    rows = torch.zeros(2, 280, device="cuda")
    with pytest.raises(RuntimeError, match="CLS_LAYER"):
        eng.reduce_codes(rows, 2)
    eng.close()


def test_predictor_loads_3x3_codes(model3, full_sd, tmp_path):
    from sylph_amd.data import SyntheticSupportSetLoader
    from sylph_amd.evaluation import inference_normalization, inference_on_support_set_dataset
    from sylph_amd.predictor import SylphPredictor
    ckpt = str(tmp_path / "model_final.pth")
    torch.save({"model": full_sd}, ckpt)
    yaml_path = str(tmp_path / "k3.yaml")
    with open(yaml_path, "w") as f:
        f.write('_BASE_: "sylph://COCO-Detection/Meta-FCOS/Meta-FCOS-finetune.yaml"\n'
                'MODEL:\n  META_LEARN:\n    CODE_GENERATOR:\n      CLS_LAYER: ["", "", 3]\n')
    code_dir = str(tmp_path / "codes" / "synthetic_all" / "0")
    sub = inference_normalization(model3, inference_on_support_set_dataset(model3, SyntheticSupportSetLoader(2, 1, 128, 160, seed=5)))
    os.makedirs(code_dir)
    for c in sub:
        c["class_code"] = {k: v.cpu() for k, v in c["class_code"].items()}
        c["class_code"]["cls_conv"] = c["class_code"]["cls_conv"] * 8.0
        torch.save(c, os.path.join(code_dir, f"{c['class_name']}.pth"))
    pred = SylphPredictor(yaml_path, ckpt, str(tmp_path / "codes"), test_dataset_names={"all": "synthetic_all"}, dtype="bf16")
    assert tuple(pred.class_codes["all"]["cls_conv"].shape) == (2, 256, 3, 3)
    pred.min_size, pred.max_size = 96, 160
    img = np.random.RandomState(0).randint(0, 256, size=(90, 130, 3), dtype=np.uint8)
    out = pred._call_few_shot(img, pred.class_codes["all"])["instances"]
    assert out.image_size == (90, 130) and len(out) > 0


def test_1x1_paths_equal_the_parent(golden_dir):
    """k = 1 behaves bit for bit as before: the head outputs and detections on g1 (bf16, gn_logits_kernel) and the support codes on g3
    (codegen_tail_kernel, normalize_codes_kernel; bf16 and fp32) are torch.equal to what the library of the
    commit before cg_code_ksize produced on an MI355X (g11_parent_1x1.npz, tests/golden/gen_parent_1x1_golden.py)"""
    want = np.load(os.path.join(golden_dir, "g11_parent_1x1.npz"))
    got = R.outputs_1x1(golden_dir)
    assert sorted(got) == sorted(want.files)
    for k in want.files:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), f"{k} differs from the parent's"
    assert sum(want[f"det_n5_t50_img{i}_scores"].size for i in range(2)) > 0 and float(np.abs(want["code_bf16_sup_s5"]).max()) > 0
