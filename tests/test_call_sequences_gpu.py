"""Orders of stage calls on one context (C ABI: sylph_fcos_head / sylph_fcos_head_pretrained / sylph_import_head / sylph_export_head /
sylph_import_pyramid / sylph_decode_nms).  A served image's detections must depend on the image, the weights and the class codes only,
never on what the context ran before: every sequence below drives ONE engine through a history and then compares its final decode,
field for field and bit for bit, with a FRESH engine that ran only the final step (same weights, same pyramid, same codes; identical
kernels on identical inputs are deterministic).

The decode workspace cleans itself (nms_kernel leaves the candidate counters zero), except after the fused many-way scan
(logits_scan_kernel, bf16 with more than 32 classes), whose candidates stay in the buffers so that a decode can be repeated.  A fused
head that no decode follows must still leave the counters to be cleared before the next plain scan (decode_scan_kernel appends to them
with atomicAdd): sequences 1-4 pin that.  Sequences 5 and 6 also run in fp32, where nothing is fused.

Kept apart from test_hip_parity.py: the forced-variant reruns of test_conv_variants_gpu.py select tests of that file by name."""
import os

import numpy as np
import pytest
import torch

from test_hip_parity import _cfg, _engine, _feats

pytestmark = pytest.mark.gpu

PAD_A = (128, 160)   # the golden pyramid (plan A)
PAD_B = (96, 128)    # a second batch shape (plan B): the golden levels cropped to its level sizes
FIELDS = ("pred_boxes", "scores", "pred_classes", "fpn_levels", "locations", "cand_index")
CLS_LOGITS_BIAS = "proposal_generator.fcos_head.cls_logits.bias"


@pytest.fixture(scope="module")
def g1(golden_dir):
    return np.load(os.path.join(golden_dir, "g1_head_decode.npz"))


@pytest.fixture(scope="module")
def sd():
    """The decode tests' head weights.  The 60-class cls_logits bias is raised from -log 99 (scores below the 0.05 threshold) to -2
    (sigmoid 0.12) so that sylph_fcos_head_pretrained alone gives detections; the class-conditional steps do not read it."""
    from sylph_amd import synthetic as W
    s = dict(W.head_state_dict(seed=1, num_classes=60))
    s[CLS_LOGITS_BIAS] = torch.full_like(s[CLS_LOGITS_BIAS], -2.0)
    return s


@pytest.fixture(scope="module")
def codes(g1):
    from sylph_amd import synthetic as W
    return {"many": W.synthetic_codes(60, seed=77, scale=3.0),  # 60-way: the fused scan in bf16
            "few": {"cls_conv": torch.from_numpy(g1["n5_t50_cls_conv"]), "cls_bias": torch.from_numpy(g1["n5_t50_cls_bias"])}}


def _sizes(g1):
    return [tuple(int(v) for v in s) for s in g1["image_sizes"]]


def _pyr_b(g1):
    out, (h, w) = [], (PAD_B[0] // 8, PAD_B[1] // 8)
    for f in _feats(g1):
        out.append(f[:, :, :h, :w].contiguous())
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return out


def _new(g1, sd, dtype, cfg=None, plan="A", **kw):
    eng = _engine(dtype, cfg if cfg is not None else _cfg(), **kw)
    eng.load_state_dict(sd)
    if plan == "A":
        eng.import_pyramid(_feats(g1), PAD_A, _sizes(g1))
    else:
        eng.import_pyramid(_pyr_b(g1), PAD_B)
    return eng


def _head(eng, c, fused):
    """One class-conditional head call; asserts whether logits_scan_kernel ran (the fused many-way head)."""
    eng.profile_enable(True)
    eng.profile_read()
    eng.head(c["cls_conv"], c["cls_bias"])
    ran = "logits_scan_kernel" in eng.profile_read()["kernels"]
    eng.profile_enable(False)
    assert ran == fused, f"logits_scan_kernel {'did not run' if fused else 'ran'} ({eng.dtype}, {c['cls_conv'].shape[0]} classes)"


def _fused_finds_candidates(g1, sd, c, dtype, cfg=None, plan="A", **decode_kw):
    """The fused step of a sequence, alone on a fresh engine: the scan ran (bf16) and found candidates -- its decode skips its own scan,
    so detections are the scan's.  Otherwise a sequence that starts with it proves nothing.  -> that decode."""
    eng = _new(g1, sd, dtype, cfg, plan)
    _head(eng, c, dtype == "bf16")
    d = eng.decode(**decode_kw)
    assert sum(x["scores"].numel() for x in d) > 0, "the fused step alone decodes nothing"
    eng.close()
    return d


def _assert_same(got, want, what):
    assert len(got) == len(want)
    assert sum(w["scores"].numel() for w in want) > 0, f"{what}: the final step alone decodes nothing -- the sequence proves nothing"
    for i, (g, w) in enumerate(zip(got, want)):
        assert g["scores"].numel() == w["scores"].numel(), \
            f"{what}: image {i}: {g['scores'].numel()} detections after the sequence, {w['scores'].numel()} on a fresh engine"
        for k in FIELDS:
            assert torch.equal(g[k], w[k]), f"{what}: image {i}: {k} differs from a fresh engine's"


def _assert_oracle(got, heads, sizes, thr=0.05, post=100):
    """The oracle decoder (predict_proposals + detector_postprocess) on the given head outputs: exact classes and locations, scores
    within 1e-5, boxes within 1e-3 (the assertions of test_many_way_fused_scan_equals_unfused)."""
    from oracle import decode as OD
    lo, rg, ct, io = [[t.cpu() for t in ts] for ts in heads]
    want = OD.predict_proposals(lo, rg, ct, io, pre_nms_thresh=thr, post_nms_topk=post)
    for i, (g, w) in enumerate(zip(got, want)):
        w = OD.detector_postprocess(w, sizes[i], sizes[i][0], sizes[i][1])
        assert g["scores"].numel() == w["scores"].numel()
        np.testing.assert_array_equal(g["pred_classes"].cpu().numpy(), w["pred_classes"].numpy())
        np.testing.assert_array_equal(g["locations"].cpu().numpy(), w["locations"].numpy())
        np.testing.assert_allclose(g["scores"].cpu().numpy(), w["scores"].numpy(), atol=1e-5)
        np.testing.assert_allclose(g["pred_boxes"].cpu().numpy(), w["pred_boxes"].numpy(), atol=1e-3)


# ------------------------------------------------------------------------------------------------ 1-4: a fused head no decode follows
def test_fused_head_export_then_plain_head(g1, sd, codes):
    """1: fused 60-way head -> export_head -> 5-way head (plain scan) -> decode == a fresh 5-way head + decode == the oracle decoder."""
    _fused_finds_candidates(g1, sd, codes["many"], "bf16")
    eng = _new(g1, sd, "bf16")
    _head(eng, codes["many"], True)
    eng.export_head()
    _head(eng, codes["few"], False)
    got = eng.decode()
    eng.close()
    fresh = _new(g1, sd, "bf16")
    _head(fresh, codes["few"], False)
    want = fresh.decode()
    _assert_same(got, want, "fused head, export, 5-way head")
    _assert_oracle(got, fresh.export_head(), _sizes(g1))


def test_fused_head_then_pretrained_head(g1, sd, codes):
    """2: fused 60-way head -> head_pretrained (the checkpoint's own 60-class cls_logits) -> decode == a fresh head_pretrained + decode."""
    _fused_finds_candidates(g1, sd, codes["many"], "bf16")
    eng = _new(g1, sd, "bf16")
    _head(eng, codes["many"], True)
    assert eng.head_pretrained() == 60
    got = eng.decode()
    eng.close()
    fresh = _new(g1, sd, "bf16")
    fresh.head_pretrained()
    _assert_same(got, fresh.decode(), "fused head, pretrained head")


def test_fused_head_export_import(g1, sd, codes):
    """3: fused 60-way head -> export_head -> import_head(those outputs) -> decode == a fresh import + decode == the oracle decoder on
    the imported tensors.  Threshold 0: every score is a candidate, so level 0 fills its 19 200-slot buffer (320 locations x 60
    classes) exactly.  (At 0.05 the stale candidates of the fused scan would be the imported ones over again, and NMS drops such
    duplicates: a decode appending to them could come out unchanged.)"""
    cfg = _cfg(**{"MODEL.FCOS.INFERENCE_TH_TEST": 0.0})
    _fused_finds_candidates(g1, sd, codes["many"], "bf16", cfg)
    eng = _new(g1, sd, "bf16", cfg)
    _head(eng, codes["many"], True)
    heads = eng.export_head()
    eng.import_head(*heads)
    got = eng.decode()
    eng.close()
    fresh = _new(g1, sd, "bf16", cfg)
    fresh.import_head(*heads)
    _assert_same(got, fresh.decode(), "fused head, export, import")
    _assert_oracle(got, heads, _sizes(g1), thr=0.0)


def test_fused_head_plan_switch_and_back(g1, sd, codes):
    """4: fused 60-way head on plan A (128x160) -> import_pyramid at 96x128 (plan B), fused head + decode there -> import_pyramid back
    at A -> 5-way head (plain scan) -> decode.  Both plans' decodes == fresh engines'."""
    _fused_finds_candidates(g1, sd, codes["many"], "bf16")
    eng = _new(g1, sd, "bf16")
    _head(eng, codes["many"], True)
    eng.import_pyramid(_pyr_b(g1), PAD_B)
    _head(eng, codes["many"], True)
    got_b = eng.decode()
    eng.import_pyramid(_feats(g1), PAD_A, _sizes(g1))
    _head(eng, codes["few"], False)
    got_a = eng.decode()
    eng.close()
    want_b = _fused_finds_candidates(g1, sd, codes["many"], "bf16", plan="B")
    _assert_same(got_b, want_b, "plan B after a fused head on plan A")
    fresh = _new(g1, sd, "bf16")
    _head(fresh, codes["few"], False)
    _assert_same(got_a, fresh.decode(), "plan A after plan B")


# ------------------------------------------------------------------------------------------------ 5-6: also in fp32 (nothing fused)
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_repeated_decode_then_plain_head(g1, sd, codes, dtype):
    """5: 60-way head -> decode -> decode (equal, and equal to a fresh engine's) -> 5-way head -> decode == a fresh 5-way head."""
    want_many = _fused_finds_candidates(g1, sd, codes["many"], dtype)
    eng = _new(g1, sd, dtype)
    _head(eng, codes["many"], dtype == "bf16")
    d1 = eng.decode()
    d2 = eng.decode()
    _assert_same(d1, want_many, "60-way head + decode")
    _assert_same(d2, d1, "repeated decode")
    _head(eng, codes["few"], False)
    got = eng.decode()
    eng.close()
    fresh = _new(g1, sd, dtype)
    _head(fresh, codes["few"], False)
    _assert_same(got, fresh.decode(), "repeated decode, 5-way head")


def _thin(lo, k=32):
    """Per image and level: every logit below the k-th largest -> -10 (sigmoid 4.5e-5): at most k candidates per (image, level) for any
    threshold above that."""
    out = []
    for t in lo:
        f = t.reshape(t.shape[0], -1)
        kth = f.topk(min(k, f.shape[1]), dim=1).values[:, -1:]
        out.append(torch.where(f >= kth, f, torch.full_like(f, -10.0)).reshape(t.shape).contiguous())
    return out


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_recovery_after_candidate_overflow(g1, sd, dtype):
    """6a: a decode that overflows a 64-slot candidate buffer raises "candidate capacity"; the same context then decodes imported head
    outputs with at most 32 candidates per (image, level) exactly as a fresh context does, and as the oracle decoder."""
    from sylph_amd import synthetic as W
    cfg = _cfg(**{"MODEL.FCOS.INFERENCE_TH_TEST": 0.011})
    c20 = W.synthetic_codes(20, seed=50, scale=2.5)
    eng = _new(g1, sd, dtype, cfg, cand_cap=64)
    _head(eng, c20, False)
    with pytest.raises(RuntimeError, match="candidate capacity"):
        eng.decode()
    lo, rg, ct, io = eng.export_head()
    heads = (_thin(lo), rg, ct, io)
    eng.import_head(*heads)
    got = eng.decode()
    eng.close()
    fresh = _new(g1, sd, dtype, cfg, cand_cap=64)
    fresh.import_head(*heads)
    _assert_same(got, fresh.decode(), "import after a candidate overflow")
    _assert_oracle(got, heads, _sizes(g1), thr=0.011)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_recovery_after_truncated_output(g1, sd, dtype):
    """6b: zero class codes (800 classes, every class of a location ties; fused in bf16): decode with max_out 300 raises "more tied
    detections than max_out" (the post-NMS keep takes every tie of the 300-th score); the next decode with max_out 5000 on the same
    context == a fresh context's."""
    cfg = _cfg(**{"MODEL.FCOS.INFERENCE_TH_TEST": 0.05, "MODEL.FCOS.POST_NMS_TOPK_TEST": 300})
    zero = {"cls_conv": torch.zeros(800, 256, 1, 1), "cls_bias": torch.zeros(800)}
    want = _fused_finds_candidates(g1, sd, zero, dtype, cfg, max_out=5000)
    assert all(w["scores"].numel() > 300 for w in want)
    eng = _new(g1, sd, dtype, cfg)
    _head(eng, zero, dtype == "bf16")
    with pytest.raises(RuntimeError, match="more tied detections than max_out"):
        eng.decode(max_out=300)
    got = eng.decode(max_out=5000)
    eng.close()
    _assert_same(got, want, "decode after a truncated one")
