"""Mixed-episode query step (sylph_fcos_head_episodes): image i of a batch is run with the class codes of episode image_episode[i].

The yardstick is the uniform step: `head(codes_e)` + `decode()` on the SAME batch, which is itself pinned to the oracle elsewhere.  For
every image the mixed step must return that run's rows bit for bit (`torch.equal`: boxes, scores, classes, levels, locations, candidate
ordinals, counts, and the exported logits in the columns of the image's own classes); no tolerance is involved.  One case compares the
fp32 head with the oracle directly.

Codes: `synthetic_codes(n, seed, scale)` as listed in CODES; with the oracle (fcos_head + predict_proposals) on a 128 x 160 randn pyramid
every one of them yields detections on every image, the 20- and 32-way sets detect classes >= 8 (beyond the 8-float narrow logits pitch)
and the two 5-way sets differ.  The tests assert those conditions on what the uniform runs return, so none of them can pass vacuously;
a decode that reports a status bit raises in `Engine.decode`."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_hip_parity import _cfg, _roienc_cfg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL, SMALL = (800, 1344), (128, 160)
FIELDS = ("pred_boxes", "scores", "pred_classes", "fpn_levels", "locations", "cand_index")
CODES = {"n1": (1, 41, 3.0), "n5": (5, 42, 3.0), "n5b": (5, 45, 3.0), "n20": (20, 43, 2.5), "n32": (32, 44, 2.5), "n60": (60, 46, 2.0)}
CLS_LOGITS_BIAS = "proposal_generator.fcos_head.cls_logits.bias"


def _levels(hw):
    out, (h, w) = [], (hw[0] // 8, hw[1] // 8)
    for _ in range(5):
        out.append((h, w))
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return out


def _pyramid(B, hw, seed=5):
    """B distinct images: a randn pyramid with bf16-representable values (the same numbers in every dtype)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.randn(B, 256, h, w, generator=g, device="cuda").bfloat16().float() for h, w in _levels(hw)]


def _code(name, c=256):
    from sylph_amd import synthetic as W
    n, seed, scale = CODES[name]
    return {k: v.cuda() for k, v in W.synthetic_codes(n, c=c, seed=seed, scale=scale).items()}


def _pairs(codes):
    return [(c["cls_conv"], c["cls_bias"]) for c in codes]


def _sd(seed=3, **kw):
    from sylph_amd import synthetic as W
    return W.head_state_dict(seed=seed, **kw)


def _new(dtype, feats, hw, sd=None, cfg=None):
    from sylph_amd.engine import Engine
    eng = Engine(cfg if cfg is not None else _cfg(), dtype=dtype)
    eng.load_state_dict(sd if sd is not None else _sd())
    eng.import_pyramid(feats, hw)
    return eng


def _same(got, want, what):
    assert got["scores"].numel() == want["scores"].numel(), f"{what}: {got['scores'].numel()} detections, expected {want['scores'].numel()}"
    for k in FIELDS:
        assert torch.equal(got[k], want[k]), f"{what}: {k} differs"


def _uniform_runs(eng, codes, image_episode, export=True):
    """head(codes_e) + decode() [+ export_head()] on the current batch for every episode that has images -> per image the rows of its
    own episode's run.  Asserts that every image has a detection under its episode."""
    dets, heads = [None] * len(image_episode), [None] * len(image_episode)
    for e, c in enumerate(codes):
        mine = [i for i, v in enumerate(image_episode) if v == e]
        if not mine:
            continue
        eng.head(c["cls_conv"], c["cls_bias"])
        d = eng.decode()
        h = eng.export_head() if export else None
        for i in mine:
            assert d[i]["scores"].numel() > 0, f"uniform run of episode {e}: image {i} has no detection -- the comparison proves nothing"
            dets[i] = d[i]
            if export:
                heads[i] = [[t[i].clone() for t in ts] for ts in h]
    return dets, heads


def _check_mixed(eng, codes, image_episode, export=True, what="mixed"):
    """The mixed step against the uniform runs of its episodes on the same engine and batch -> (mixed detections, uniform detections)."""
    want, want_heads = _uniform_runs(eng, codes, image_episode, export)
    eng.head_episodes(_pairs(codes), image_episode)
    got = eng.decode()
    for i, e in enumerate(image_episode):
        _same(got[i], want[i], f"{what}: image {i} (episode {e})")
        n = codes[e]["cls_conv"].shape[0]
        assert int(got[i]["pred_classes"].max()) < n
    if export:
        lo, rg, ct, io = eng.export_head()
        nmax = max(c["cls_conv"].shape[0] for c in codes)
        for i, e in enumerate(image_episode):
            n = codes[e]["cls_conv"].shape[0]
            for l in range(len(lo)):
                assert lo[l].shape[1] == nmax
                assert torch.equal(lo[l][i, :n], want_heads[i][0][l][:n]), f"{what}: image {i} level {l}: logits of its {n} classes differ"
                for name, g, w in (("reg", rg, 1), ("ctr", ct, 2), ("iou", io, 3)):
                    assert torch.equal(g[l][i], want_heads[i][w][l]), f"{what}: image {i} level {l}: {name} differs"
    return got, want


def _assert_wide_classes(dets, image_episode, episodes):
    """the 20- / 32-way episodes detect a class beyond the narrow 8-float logits pitch"""
    for e in episodes:
        top = max(int(dets[i]["pred_classes"].max()) for i, v in enumerate(image_episode) if v == e)
        assert top >= 8, f"episode {e}: highest detected class {top}: columns >= 8 are not exercised"


def _assert_distinguishes(eng, image):
    """two 5-way episodes give different detections on one image: the comparisons can tell whose codes were used"""
    out = []
    for name in ("n5", "n5b"):
        c = _code(name)
        eng.head(c["cls_conv"], c["cls_bias"])
        out.append(eng.decode()[image])
    a, b = out
    assert a["scores"].numel() > 0 and b["scores"].numel() > 0
    assert a["scores"].numel() != b["scores"].numel() or not all(torch.equal(a[k], b[k]) for k in FIELDS), \
        "the two 5-way code sets give the same detections"


# ------------------------------------------------------------------------------------------------ 1: bf16, production shape
def test_mixed_equals_uniform_bf16_800x1344():
    """B = 8 distinct images, four episodes N = 1, 5, 20, 32, interleaved: the single fused launch (every N <= 32)."""
    codes = [_code(k) for k in ("n1", "n5", "n20", "n32")]
    ie = [0, 1, 2, 3, 3, 2, 1, 0]
    eng = _new("bf16", _pyramid(8, FULL), FULL)
    got, _ = _check_mixed(eng, codes, ie)
    _assert_wide_classes(got, ie, (2, 3))
    _assert_distinguishes(eng, 1)
    eng.close()


# ------------------------------------------------------------------------------------------------ 2: f32, f32s
@pytest.mark.parametrize("dtype", ["f32", "f32s"])
def test_mixed_equals_uniform_fp32(dtype):
    """conv_igemm over per-episode tile sub-lists (no fused GroupNorm in fp32 storage): equal by construction, checked all the same."""
    codes = [_code(k) for k in ("n1", "n5", "n20", "n32")]
    ie = [0, 1, 2, 3, 3, 2, 1, 0]
    eng = _new(dtype, _pyramid(8, SMALL), SMALL)
    got, _ = _check_mixed(eng, codes, ie, what=dtype)
    _assert_wide_classes(got, ie, (2, 3))
    _assert_distinguishes(eng, 1)
    eng.close()


# ------------------------------------------------------------------------------------------------ 3: the oracle, f32
def test_mixed_head_f32_matches_oracle_and_decoder():
    """oracle.head.fcos_head per image with that image's codes: head outputs within 1e-3 (the fp32 bar); the oracle decoder on the HIP
    head outputs of each image picks the candidates the mixed decode returned."""
    from oracle import decode as OD, head as OH
    codes = [_code(k) for k in ("n1", "n5", "n20", "n32")]
    ie = [3, 1, 0, 2]
    feats = _pyramid(4, SMALL)
    sd = _sd()
    eng = _new("f32", feats, SMALL, sd=sd)
    eng.head_episodes(_pairs(codes), ie)
    got = eng.decode()
    heads = [[t.cpu() for t in ts] for ts in eng.export_head()]
    worst = 0.0
    for i, e in enumerate(ie):
        n = codes[e]["cls_conv"].shape[0]
        want = OH.fcos_head([f[i:i + 1].cpu() for f in feats], sd, {k: v.cpu() for k, v in codes[e].items()})
        mine = [[t[i:i + 1, :n] for t in heads[0]]] + [[t[i:i + 1] for t in ts] for ts in heads[1:]]
        for gl, wl in zip(mine, want):
            for g, w in zip(gl, wl):
                assert g.shape == w.shape
                worst = max(worst, float((g.double() - w.double()).abs().max()) / max(1.0, float(w.abs().max())))
        ref = OD.predict_proposals(*mine)[0]
        ref = OD.detector_postprocess(ref, SMALL, SMALL[0], SMALL[1])
        d = got[i]
        assert d["scores"].numel() == ref["scores"].numel() > 0, f"image {i}"
        np.testing.assert_array_equal(d["pred_classes"].cpu().numpy(), ref["pred_classes"].numpy())
        np.testing.assert_array_equal(d["locations"].cpu().numpy(), ref["locations"].numpy())
        np.testing.assert_array_equal(d["fpn_levels"].cpu().numpy(), ref["fpn_levels"].numpy())
        np.testing.assert_allclose(d["scores"].cpu().numpy(), ref["scores"].numpy(), atol=1e-5)
        np.testing.assert_allclose(d["pred_boxes"].cpu().numpy(), ref["pred_boxes"].numpy(), atol=1e-3)
    print(f"worst head difference from the oracle: {worst:.2e}")
    assert worst <= 1e-3
    eng.close()


# ------------------------------------------------------------------------------------------------ 4: per-episode launches
def _kernels(eng, fn):
    eng.profile_enable(True)
    eng.profile_read()
    fn()
    k = {n: v["launches"] for n, v in eng.profile_read()["kernels"].items()}
    eng.profile_enable(False)
    return k


def test_fallback_many_way_next_to_few_way_bf16():
    """A 60-way episode (fused conv + scan, which leaves candidates instead of logits) next to a 5-way one (fused GroupNorm + conv):
    the decode scans the 5-way images only; the export runs the 60-way conv on demand."""
    codes = [_code("n60"), _code("n5")]
    ie = [0, 1, 1, 0]
    eng = _new("bf16", _pyramid(4, SMALL), SMALL)
    _check_mixed(eng, codes, ie, what="60-way + 5-way")
    k = _kernels(eng, lambda: eng.head_episodes(_pairs(codes), ie))
    assert k.get("logits_scan_kernel") == 1 and k.get("gn_logits_kernel") == 1 and "gn_logits_episodes_kernel" not in k, k
    first = eng.decode()
    again = eng.decode()  # the scan's candidates stay, the 5-way images are scanned again
    for i in range(4):
        _same(again[i], first[i], f"repeated decode: image {i}")
    eng.close()


_FUSE_SCAN_OFF_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import test_mixed_episodes_gpu as T
codes, ie = [T._code("n60"), T._code("n5")], [0, 1, 1, 0]
eng = T._new("bf16", T._pyramid(4, T.SMALL), T.SMALL)
T._check_mixed(eng, codes, ie, what="SYLPH_FUSE_SCAN=0")  # (every image has detections: asserted on the uniform runs)
few = T._kernels(eng, lambda: eng.head(codes[1]["cls_conv"], codes[1]["cls_bias"]))
uni = T._kernels(eng, lambda: eng.head(codes[0]["cls_conv"], codes[0]["cls_bias"]))
mix = T._kernels(eng, lambda: eng.head_episodes(T._pairs(codes), ie))
print("uniform 5-way head:", few, "\nuniform 60-way head:", uni, "\nmixed head:", mix)
assert "logits_scan_kernel" not in uni and "logits_scan_kernel" not in mix
tower = few.get("conv_igemm_kernel", 0)  # the 5-way head's class-conditional conv is gn_logits_kernel: these are its tower layers
assert few.get("gn_logits_kernel") == 1 and "logits_scan_kernel" not in few
assert uni.get("conv_igemm_kernel") == tower + 1 and "gn_logits_kernel" not in uni
assert mix.get("gn_logits_kernel") == 1 and mix.get("conv_igemm_kernel") == tower + 1
eng.close()
"""


def test_mixed_head_follows_fuse_scan_switch():
    """SYLPH_FUSE_SCAN=0 (one fresh child process): the 60-way episode of a mixed head runs what the uniform 60-way head runs then, the
    GroupNorm apply + conv_igemm, behind the 5-way episode's gn_logits_kernel (which reads the tower output before that in-place apply);
    no fused scan in either head, and the mixed step still equals the uniform runs bit for bit, exported logits included.  At this size
    the tower layers run conv_igemm_kernel too (8 launches), so "the class-conditional conv_igemm ran once" is counted against the
    uniform 5-way head, whose class-conditional conv is gn_logits_kernel.  The smallest batch with a few-way and a many-way episode
    on more than one image each."""
    r = subprocess.run([sys.executable, "-c", _FUSE_SCAN_OFF_CHILD, os.path.join(ROOT, "sylph-few-shot-detection_amd"), os.path.join(ROOT, "tests")],
                       env=dict(os.environ, SYLPH_FUSE_SCAN="0"), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_fallback_norm_none_bf16():
    codes = [_code(k) for k in ("n5", "n20", "n5b")]
    ie = [0, 1, 2, 1]
    cfg = _cfg(**{"MODEL.FCOS.NORM": "none"})
    eng = _new("bf16", _pyramid(4, SMALL), SMALL, sd=_sd(norm="none"), cfg=cfg)
    _check_mixed(eng, codes, ie, what="NORM none")
    k = _kernels(eng, lambda: eng.head_episodes(_pairs(codes), ie))
    assert "gn_logits_episodes_kernel" not in k and "gn_logits_kernel" not in k, k
    eng.close()


def test_fallback_roi_encoder_512_channel_codes():
    """CondConvBlock codes (k = 2 chunks of 256 channels) fold into one 256-channel code per class on the host, per episode."""
    from sylph_amd import synthetic as W
    sd = dict(_sd())
    sd.update(W.roi_encoder_state_dict(seed=4))
    codes = [_code("n5", c=512), _code("n20", c=512)]
    ie = [1, 0, 0, 1]
    eng = _new("bf16", _pyramid(4, SMALL), SMALL, sd=sd, cfg=_roienc_cfg())
    assert eng.is_roi_encoder
    _check_mixed(eng, codes, ie, what="ROIEncoder")
    eng.close()


# ------------------------------------------------------------------------------------------------ 5: permutation
def test_permuting_images_and_episodes_permutes_results():
    codes = [_code(k) for k in ("n1", "n5", "n20", "n32", "n5b")]
    ie = [0, 1, 2, 3, 4, 1]
    feats = _pyramid(6, SMALL)
    eng = _new("bf16", feats, SMALL)
    eng.head_episodes(_pairs(codes), ie)
    base = eng.decode()
    assert all(d["scores"].numel() > 0 for d in base)
    perm = [4, 2, 5, 0, 3, 1]
    eng.import_pyramid([f[perm].contiguous() for f in feats], SMALL)
    eng.head_episodes(_pairs(codes), [ie[p] for p in perm])
    got = eng.decode()
    for j, p in enumerate(perm):
        _same(got[j], base[p], f"position {j} (image {p})")
    eng.close()


# ------------------------------------------------------------------------------------------------ 6: call sequences
def _seq_sd():
    """cls_logits bias raised so that the pretrained head alone gives detections (tests/test_call_sequences_gpu.py)"""
    s = dict(_sd(num_classes=60))
    s[CLS_LOGITS_BIAS] = torch.full_like(s[CLS_LOGITS_BIAS], -2.0)
    return s


@pytest.mark.parametrize("mix", ["few", "many"])
def test_mixed_head_then_uniform_head_then_decode(mix):
    """`many`: the mixed head ran the fused scan for its 60-way episode and no decode followed -- the uniform step after it starts from a
    cleared candidate table."""
    codes = [_code("n60" if mix == "many" else "n20"), _code("n5")]
    ie = [0, 1, 1, 0]
    feats, sd, last = _pyramid(4, SMALL), _seq_sd(), _code("n5b")
    eng = _new("bf16", feats, SMALL, sd=sd)
    eng.head_episodes(_pairs(codes), ie)
    eng.head(last["cls_conv"], last["cls_bias"])
    got = eng.decode()
    eng.close()
    fresh = _new("bf16", feats, SMALL, sd=sd)
    fresh.head(last["cls_conv"], last["cls_bias"])
    want = fresh.decode()
    fresh.close()
    assert sum(w["scores"].numel() for w in want) > 0
    for i in range(4):
        _same(got[i], want[i], f"image {i}")


@pytest.mark.parametrize("mix", ["few", "many"])
def test_mixed_head_then_pretrained_head_then_decode(mix):
    codes = [_code("n60" if mix == "many" else "n20"), _code("n5")]
    ie = [0, 1, 1, 0]
    feats, sd = _pyramid(4, SMALL), _seq_sd()
    eng = _new("bf16", feats, SMALL, sd=sd)
    eng.head_episodes(_pairs(codes), ie)
    eng.head_pretrained()
    got = eng.decode()
    eng.close()
    fresh = _new("bf16", feats, SMALL, sd=sd)
    fresh.head_pretrained()
    want = fresh.decode()
    fresh.close()
    assert sum(w["scores"].numel() for w in want) > 0
    for i in range(4):
        _same(got[i], want[i], f"image {i}")


def test_second_decode_after_mixed_head_repeats_the_first():
    codes = [_code(k) for k in ("n1", "n5", "n20", "n32")]
    ie = [0, 1, 2, 3]
    eng = _new("bf16", _pyramid(4, SMALL), SMALL)
    eng.head_episodes(_pairs(codes), ie)
    first = eng.decode()
    again = eng.decode()
    assert all(d["scores"].numel() > 0 for d in first)
    for i in range(4):
        _same(again[i], first[i], f"image {i}")
    eng.close()


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_single_episode_equals_uniform_head(dtype):
    c = _code("n20")
    eng = _new(dtype, _pyramid(3, SMALL), SMALL)
    _check_mixed(eng, [c], [0, 0, 0], what=f"E = 1 ({dtype})")
    eng.close()


def test_episode_errors():
    c = _code("n5")
    eng = _new("bf16", _pyramid(2, SMALL), SMALL)
    with pytest.raises(ValueError):
        eng.head_episodes(_pairs([c]), [0])          # one entry for two images
    with pytest.raises(ValueError):
        eng.head_episodes(_pairs([c]), [0, 1])       # episode 1 does not exist
    with pytest.raises(ValueError):
        eng.head_episodes([], [0, 0])
    eng.head_episodes(_pairs([c, _code("n20")]), [0, 0])  # an episode that no image uses is allowed
    assert all(d["scores"].numel() > 0 for d in eng.decode())
    L, ctx = eng.L, eng._ctx
    from sylph_amd.engine import _iarr, _ptr
    w = c["cls_conv"].reshape(5, 256).contiguous()
    assert L.sylph_fcos_head_episodes(ctx, 0, _ptr(w), None, _iarr([5]), _iarr([0, 0])) != 0
    assert L.sylph_fcos_head_episodes(ctx, 1, _ptr(w), None, _iarr([0]), _iarr([0, 0])) != 0
    assert L.sylph_fcos_head_episodes(ctx, 1, _ptr(w), None, _iarr([5]), _iarr([0, 1])) != 0
    assert L.sylph_fcos_head_episodes(ctx, 1, None, None, _iarr([5]), _iarr([0, 0])) != 0
    eng.close()


# ------------------------------------------------------------------------------------------------ 7: the model API
def test_model_accepts_one_class_code_dict_per_input():
    from sylph_amd import synthetic as W
    from sylph_amd.runner import MetaFCOSRunner, create_cfg
    r = MetaFCOSRunner()
    cfg = create_cfg(r.get_default_cfg(), "sylph://COCO-Detection/Meta-FCOS/Meta-FCOS-finetune.yaml")
    model = r.build_model(cfg, dtype="bf16")
    model.load_state_dict(W.synthetic_state_dict(0, depth=50))
    model.eval()
    batch = [{"image": im, "height": 120, "width": 150} for im in W.synthetic_images(4, 128, 160, seed=9)]
    d0, d1, d2 = _code("n5"), _code("n5b"), _code("n20")
    kw = dict(run_type="meta_learn_test_instance")
    got = model(batch, class_code=[d0, d1, d0, d2], **kw)
    assert len(got) == 4
    differ = False
    for k, d in enumerate((d0, d1, d2)):
        want = model(batch, class_code=d, **kw)
        for i, dd in enumerate((d0, d1, d0, d2)):
            g, w = got[i]["instances"], want[i]["instances"]
            if dd is d:
                assert len(w) > 0, f"uniform call {k}: image {i} has no detection"
                assert g.image_size == w.image_size and len(g) == len(w)
                for f in ("scores", "pred_classes", "locations", "fpn_levels"):
                    assert torch.equal(getattr(g, f), getattr(w, f)), f"image {i}: {f}"
                assert torch.equal(g.pred_boxes.tensor, w.pred_boxes.tensor), f"image {i}: pred_boxes"
            elif i == 0:
                differ = differ or len(g) != len(w) or not torch.equal(g.scores, w.scores)
    assert differ, "image 0 gets the same detections under other episodes' codes"
    with pytest.raises(ValueError):
        model(batch, class_code=[d0, d1], **kw)
    with pytest.raises(ValueError):
        model(batch, class_code=[d0, None, d0, d2], **kw)


# ------------------------------------------------------------------------------------------------ 8: the headline batch
def test_headline_batch_192_images_192_episodes():
    """B = 192 at 800 x 1344: image i is a copy of distinct image i % 4 and has an episode of its own whose codes are a COPY (separate
    tensors) of 5-way set (i // 4) % 8.  Every image equals the image at position i % 32, and positions 0-31 equal the uniform runs."""
    from sylph_amd import synthetic as W
    NB = 192
    sets = [{k: v.cuda() for k, v in W.synthetic_codes(5, seed=100 + s, scale=3.0).items()} for s in range(8)]
    four = _pyramid(4, FULL, seed=7)
    eng = _new("bf16", [f.repeat(NB // 4, 1, 1, 1) for f in four], FULL)
    del four
    codes = [{k: v.clone() for k, v in sets[(i // 4) % 8].items()} for i in range(NB)]
    k = _kernels(eng, lambda: eng.head_episodes(_pairs(codes), list(range(NB))))
    assert k.get("gn_logits_episodes_kernel") == 1 and "gn_logits_kernel" not in k, k
    got = eng.decode()
    assert len(got) == NB
    for i in range(32, NB):
        _same(got[i], got[i % 32], f"image {i} vs position {i % 32}")
    for s in range(8):
        eng.head(sets[s]["cls_conv"], sets[s]["cls_bias"])
        want = eng.decode()
        for p in range(32):
            if (p // 4) % 8 == s:
                assert want[p]["scores"].numel() > 0, f"uniform run of code set {s}: image {p} has no detection"
                _same(got[p], want[p], f"position {p} vs the uniform run of code set {s}")
    # the code sets are told apart: image 0 under set 0 and the same image (position 4) under set 1
    assert got[0]["scores"].numel() != got[4]["scores"].numel() or not all(torch.equal(got[0][f], got[4][f]) for f in FIELDS)
    eng.close()


# ------------------------------------------------------------------------------------------------ 9: one launch
@pytest.mark.parametrize("E", [2, 8])
def test_one_class_conditional_launch_whatever_the_episode_count(E):
    names = ["n5", "n20", "n1", "n32", "n5b", "n5", "n20", "n32"][:E]
    codes = [_code(k) for k in names]
    ie = [i % E for i in range(8)]
    eng = _new("bf16", _pyramid(8, SMALL), SMALL)
    uni = _kernels(eng, lambda: (eng.head(codes[0]["cls_conv"], codes[0]["cls_bias"]), eng.decode()))
    mix = _kernels(eng, lambda: (eng.head_episodes(_pairs(codes), ie), eng.decode()))
    assert uni.get("gn_logits_kernel") == 1
    assert mix.get("gn_logits_episodes_kernel") == 1, mix
    assert "gn_logits_kernel" not in mix and "logits_scan_kernel" not in mix, mix
    assert mix.get("conv_igemm_kernel", 0) <= uni.get("conv_igemm_kernel", 0), (mix, uni)
    assert sum(mix.values()) == sum(uni.values()), (mix, uni)
    eng.close()
