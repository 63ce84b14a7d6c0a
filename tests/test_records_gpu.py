"""Query records (sylph_record_store / sylph_record_load): class codes scored on stored tower outputs.

The yardstick is always the fresh step: the head entry + its decode (+ `export_head`) on the SAME engine and batch, which is pinned to the
oracle elsewhere.  Scoring a record must return that run bit for bit (`torch.equal` on every field of FIELDS, on the counts and on the
exported logits and predictions); no tolerance is involved.  Every case first asserts that each image has a detection in the yardstick
run, so that none can pass vacuously; a decode that reports a status bit raises in `Engine.decode`.

Batches: three or four images at 128 x 160 through `Engine.import_pyramid`: 428 rows per image (20 x 16 + 10 x 8 + ... + 1 x 2), so every
segment but the first is shorter than a 128-row tile and the first is no multiple of one."""
import os
import subprocess
import sys

import pytest
import torch

import spatial_codes_ref as R3
from test_hip_parity import _cfg, _roienc_cfg
from test_mixed_episodes_gpu import FIELDS, SMALL, _code, _kernels, _new, _pairs, _pyramid, _same, _sd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED = [(128, 160), (100, 150), (64, 96)]
CLS_LOGITS_BIAS = "proposal_generator.fcos_head.cls_logits.bias"
# the profiled kernels of a class-conditional conv (the decode's are not profiled): all that scoring a record may launch
COND = {"gn_logits_kernel", "logits_scan_kernel", "gn_logits_sets_kernel", "gn_logits_episodes_kernel", "gn_apply_partials_kernel",
        "conv_igemm_kernel", "gn_cond3x3_kernel"}


# ------------------------------------------------------------------------------------------------ runs: head entry + decode + export
def _uniform(c, export=True):
    def run(eng):
        eng.head(c["cls_conv"], c["cls_bias"])
        return [eng.decode()], (eng.export_head() if export else None), None
    return run


def _sets(codes):
    def run(eng):
        eng.head_code_sets(_pairs(codes))
        return eng.decode_code_sets(), eng.export_head(), None
    return run


def _episodes(codes, ie):
    def run(eng):
        eng.head_episodes(_pairs(codes), ie)
        return [eng.decode()], eng.export_head(), [codes[e]["cls_conv"].shape[0] for e in ie]
    return run


def _pretrained(eng):
    eng.head_pretrained()
    return [eng.decode()], eng.export_head(), None


def _assert_detects(dets, what):
    for g, per_image in enumerate(dets):
        for i, d in enumerate(per_image):
            assert d["scores"].numel() > 0, f"{what}: yardstick run {g}, image {i} has no detection -- the comparison proves nothing"


def _equal_runs(got, want, what):
    (gd, gh, own), (wd, wh, _) = got, want
    assert len(gd) == len(wd)
    for g, (a, b) in enumerate(zip(gd, wd)):
        assert len(a) == len(b)
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{what}: run {g}, image {i}")
    if wh is None:
        return
    for t, name in enumerate(("logits", "reg", "ctr", "iou")):
        for l, (x, y) in enumerate(zip(gh[t], wh[t])):
            if t == 0 and own is not None:  # a mixed head: the logits beyond an image's own classes are unspecified
                for i, n in enumerate(own):
                    assert torch.equal(x[i, :n], y[i, :n]), f"{what}: {name}, level {l}, image {i}"
            else:
                assert torch.equal(x, y), f"{what}: {name}, level {l}"


def _record_of(eng, feats, sizes=None, after=None):
    """a record of `feats` as the fresh batch: after towers(), or after the head call `after`"""
    eng.import_pyramid(feats, SMALL, sizes)
    if after is None:
        eng.towers()
    else:
        after(eng)
    return eng.store_record()


def _check(eng, feats, run, what, sizes=None, after=None, dirty=None):
    """yardstick on the fresh batch; a record of the same batch; the plan's buffers overwritten by another batch; the record scored"""
    eng.import_pyramid(feats, SMALL, sizes)
    want = run(eng)
    _assert_detects(want[0], what)
    rec = _record_of(eng, feats, sizes, after)
    eng.import_pyramid(dirty if dirty is not None else [torch.zeros_like(f) for f in feats], SMALL)
    eng.towers()
    eng.load_record(rec)
    got = run(eng)
    _equal_runs(got, want, what)
    again = run(eng)  # nothing that scored it wrote into it
    _equal_runs(again, want, what + " (second score)")
    rec.close()
    return want


# ------------------------------------------------------------------------------------------------ 1: routes
@pytest.fixture(scope="module")
def feats():
    return _pyramid(3, SMALL)


@pytest.fixture(scope="module")
def bf16(feats):
    eng = _new("bf16", feats, SMALL)
    yield eng
    eng.close()


@pytest.mark.parametrize("name", ["n5", "n20", "n32", "n60"])
def test_uniform_head_routes_bf16(bf16, feats, name):
    """n5: the fused GroupNorm + conv at the narrow logits pitch; n20 / n32: the same kernel, 32 columns; n60: the fused scan (whose
    logits export restores the record and runs the unfused conv).  Ragged image sizes for n20."""
    want = _check(bf16, feats, _uniform(_code(name)), name, sizes=RAGGED if name == "n20" else None)
    if name in ("n20", "n32"):
        top = max(int(d["pred_classes"].max()) for d in want[0][0])
        assert top >= 8, f"{name}: highest detected class {top}: columns >= 8 are not exercised"


def test_record_stored_after_a_head_call(bf16, feats):
    """a record may be stored after any head entry that left the tower output as the streaming kernels read it"""
    c = _code("n5")
    _check(bf16, feats, _uniform(_code("n20")), "stored after a 5-way head", after=lambda e: e.head(c["cls_conv"], c["cls_bias"]))


def test_code_sets_head(bf16, feats):
    _check(bf16, feats, _sets([_code(k) for k in ("n5", "n5b", "n1", "n20")]), "code sets")


def test_mixed_episode_head(bf16):
    four = _pyramid(4, SMALL, seed=6)
    _check(bf16, four, _episodes([_code("n60"), _code("n5")], [0, 1, 1, 0]), "60-way next to 5-way")
    _check(bf16, four, _episodes([_code("n5"), _code("n20"), _code("n5b")], [0, 1, 2, 1]), "few-way episodes, one launch")


def test_pretrained_head(feats):
    sd = dict(_sd(num_classes=60))
    sd[CLS_LOGITS_BIAS] = torch.full_like(sd[CLS_LOGITS_BIAS], -2.0)  # so that the pretrained head alone gives detections
    eng = _new("bf16", feats, SMALL, sd=sd)
    _check(eng, feats, _pretrained, "pretrained")
    eng.close()


def test_3x3_codes(feats):
    cfg = _cfg(**{"MODEL.META_LEARN.CODE_GENERATOR.CLS_LAYER": ["", "", 3]})
    eng = _new("bf16", feats, SMALL, cfg=cfg)
    c = {k: v.cuda() for k, v in R3.spatial_codes(5, 72, 1.5).items()}
    _check(eng, feats, _uniform(c), "3x3 codes")
    eng.close()


@pytest.mark.parametrize("dtype", ["f32", "f32s"])
def test_fp32_storage(feats, dtype):
    eng = _new(dtype, feats, SMALL)
    _check(eng, feats, _uniform(_code("n5")), dtype)
    _check(eng, feats, _sets([_code("n5"), _code("n20")]), dtype + " code sets")
    eng.close()


def test_norm_none(feats):
    eng = _new("bf16", feats, SMALL, sd=_sd(norm="none"), cfg=_cfg(**{"MODEL.FCOS.NORM": "none"}))
    _check(eng, feats, _uniform(_code("n5")), "NORM none")
    eng.close()


def test_roi_encoder_config(feats):
    from sylph_amd import synthetic as W
    sd = dict(_sd())
    sd.update(W.roi_encoder_state_dict(seed=4))
    eng = _new("bf16", feats, SMALL, sd=sd, cfg=_roienc_cfg())
    assert eng.is_roi_encoder
    _check(eng, feats, _uniform(_code("n5", c=512)), "ROIEncoder")
    eng.close()


# ------------------------------------------------------------------------------------------------ 2: no network in the score
@pytest.mark.parametrize("name", ["n5", "n60"])
def test_scoring_a_record_launches_no_tower(bf16, feats, name):
    c = _code(name)
    step = lambda: (bf16.head(c["cls_conv"], c["cls_bias"]), bf16.decode())
    bf16.import_pyramid(feats, SMALL)
    fresh = _kernels(bf16, step)
    rec = bf16.store_record()
    bf16.load_record(rec)
    scored = _kernels(bf16, step)
    print("fresh:", fresh, "\nrecord:", scored)
    towers = set(fresh) - set(scored)
    # the fresh call ran kernels the record score did not: at this size the tower layers are conv_igemm launches, the prediction pass
    # gn_taps (at 800 x 1344 the towers run conv_hpipe) ...
    assert any(k.startswith("conv_") for k in towers) and "gn_taps_kernel+tap_gather_kernel" in towers, (fresh, scored)
    assert set(scored) <= COND and set(scored) <= set(fresh), scored     # ... and the score ran class-conditional kernels only,
    cond = "gn_logits_kernel" if name == "n5" else "logits_scan_kernel"
    assert scored == {cond: 1}, scored                                   # one launch, the streaming one, no copy of the features
    assert fresh.get(cond) == 1
    rec.close()


# ------------------------------------------------------------------------------------------------ 3: immutability and order
def test_one_record_scored_in_many_ways(bf16, feats):
    n5, n60 = _code("n5"), _code("n60")
    sets = [_code(k) for k in ("n5", "n5b", "n1", "n20")]
    bf16.import_pyramid(feats, SMALL)
    want5, want60, want_sets = _uniform(n5)(bf16), _uniform(n60)(bf16), _sets(sets)(bf16)
    for w, what in ((want5, "n5"), (want60, "n60"), (want_sets, "code sets")):
        _assert_detects(w[0], what)
    rec = _record_of(bf16, feats)
    bf16.load_record(rec)
    bf16.head(n60["cls_conv"], n60["cls_bias"])  # the fused scan, never decoded ...
    heads = bf16.export_head()                    # ... whose logits the unfused conv writes now, normalising a COPY of the record in place
    for t in range(4):
        for l in range(5):
            assert torch.equal(heads[t][l], want60[1][t][l]), f"export after the scan: tensor {t}, level {l}"
    first = _uniform(n5)(bf16)
    _equal_runs(first, want5, "n5 after the export")
    _equal_runs(_sets(sets)(bf16), want_sets, "code sets after n5")
    _equal_runs(_uniform(n60)(bf16), want60, "n60 after the code sets")
    last = _uniform(n5)(bf16)
    _equal_runs(last, want5, "n5 again")
    _equal_runs(last, first, "first and last n5")
    rec.close()


# ------------------------------------------------------------------------------------------------ 4: interleaving on one shape
def test_records_and_fresh_batches_interleaved(bf16, feats):
    n5, n60 = _code("n5"), _code("n60")
    X, Y, Z = feats, _pyramid(3, SMALL, seed=11), _pyramid(3, (96, 160), seed=12)
    bf16.import_pyramid(X, SMALL)
    wantX = _uniform(n5)(bf16)
    bf16.import_pyramid(Y, SMALL)
    wantY = _uniform(n5)(bf16)
    wantY60 = _uniform(n60, export=False)(bf16)
    for w, what in ((wantX, "X"), (wantY, "Y"), (wantY60, "Y 60-way")):
        _assert_detects(w[0], what)
    A = _record_of(bf16, X)
    for second_shape in (False, True):
        bf16.import_pyramid(Y, SMALL)            # full fresh steps on the record's shape: few-way ...
        _equal_runs(_uniform(n5)(bf16), wantY, "Y few-way")
        bf16.import_pyramid(Y, SMALL)
        bf16.head(n60["cls_conv"], n60["cls_bias"])  # ... and many-way with no decode: the scan's candidates stay counted
        if second_shape:
            bf16.import_pyramid(Z, (96, 160))
            bf16.head(n5["cls_conv"], n5["cls_bias"])
            bf16.decode()
        bf16.load_record(A)
        _equal_runs(_uniform(n5)(bf16), wantX, "record A after fresh steps")
        bf16.head(n60["cls_conv"], n60["cls_bias"])  # a many-way scan on the record that is never decoded ...
        bf16.import_pyramid(Y, SMALL)                # ... then a few-way head on a fresh batch of the same shape: clean counters
        _equal_runs(_uniform(n5)(bf16), wantY, "Y again")
        _equal_runs(_uniform(n60, export=False)(bf16), wantY60, "Y 60-way again")
    Bm = _record_of(bf16, Y)                         # two records of one shape, scored alternately
    for _ in range(2):
        bf16.load_record(A)
        _equal_runs(_uniform(n5)(bf16), wantX, "A, alternating")
        bf16.load_record(Bm)
        _equal_runs(_uniform(n5)(bf16), wantY, "B, alternating")
        _equal_runs(_uniform(n60, export=False)(bf16), wantY60, "B 60-way, alternating")
    A.close()
    Bm.close()


# ------------------------------------------------------------------------------------------------ 5: plan eviction
_EVICTION_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import torch
import test_records_gpu as T
c = T._code("n5")
X = T._pyramid(3, T.SMALL)
eng = T._new("bf16", X, T.SMALL)
want = T._uniform(c)(eng)
T._assert_detects(want[0], "eviction")
eng.import_pyramid(X, T.SMALL)
eng.towers()
before = eng.device_bytes()
rec = eng.store_record()
assert rec.nbytes > 0 and eng.device_bytes() == before + rec.nbytes, (before, rec.nbytes, eng.device_bytes())
for hw in ((64, 96), (96, 96), (96, 160), (64, 160)):  # more shapes than SYLPH_MAX_PLANS = 2 keeps: the record's plan is evicted
    eng.import_pyramid(T._pyramid(2, hw, seed=13), hw)
    eng.head(c["cls_conv"], c["cls_bias"])
    eng.decode()
eng.load_record(rec)
T._equal_runs(T._uniform(c)(eng), want, "after eviction")
held = eng.device_bytes()
rec.close()
assert eng.device_bytes() == held - rec.nbytes, (held, rec.nbytes, eng.device_bytes())
eng.close()
"""


def test_record_survives_plan_eviction():
    r = subprocess.run([sys.executable, "-c", _EVICTION_CHILD, os.path.join(ROOT, "sylph-few-shot-detection_amd"), os.path.join(ROOT, "tests")],
                       env=dict(os.environ, SYLPH_MAX_PLANS="2"), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ 6: refusals
def test_refusals(feats):
    from sylph_amd import synthetic as W
    n5, n60 = _code("n5"), _code("n60")
    eng = _new("bf16", feats, SMALL)
    with pytest.raises(RuntimeError, match="towers have not run"):
        eng.store_record()                                   # a fresh batch, no towers yet
    eng.towers()
    with pytest.raises(RuntimeError, match="sylph_fcos_head must be called first"):
        eng.decode()                                         # towers alone leave nothing to decode
    with pytest.raises(RuntimeError, match="sylph_fcos_head must be called first"):
        eng.export_head()
    rec = eng.store_record()
    eng.import_pyramid(feats, SMALL)
    eng.head(n60["cls_conv"], n60["cls_bias"])
    eng.export_head()                                        # the unfused conv has normalised the tower output in place
    with pytest.raises(RuntimeError, match="GroupNorm in place"):
        eng.store_record()
    eng.load_record(rec)
    with pytest.raises(RuntimeError, match="sylph_fcos_head must be called first"):
        eng.decode()                                         # loading a record leaves nothing to decode either
    with pytest.raises(RuntimeError, match="query record"):
        eng.codegen(W.synthetic_boxes(3, 128, 160, seed=70))
    with pytest.raises(RuntimeError, match="sylph_export_pyramid.*query record"):
        eng.export_pyramid()
    with pytest.raises(RuntimeError, match="sylph_backbone_fpn.*query record"):
        eng.backbone()
    with pytest.raises(RuntimeError, match="sylph_fcos_towers.*query record"):
        eng.towers()
    with pytest.raises(RuntimeError, match="query record already"):
        eng.store_record()
    other = _new("f32", feats, SMALL)
    with pytest.raises(RuntimeError, match="dtype bf16"):
        other.load_record(rec)
    other.close()
    other = _new("bf16", feats, SMALL, sd=_sd(norm="none"), cfg=_cfg(**{"MODEL.FCOS.NORM": "none"}))
    with pytest.raises(RuntimeError, match="another sylph_config"):
        other.load_record(rec)
    other.close()
    eng.head(n5["cls_conv"], n5["cls_bias"])                 # the refusals left the record current and intact
    assert all(d["scores"].numel() > 0 for d in eng.decode())
    rec.close()
    with pytest.raises(RuntimeError, match="closed"):
        eng.load_record(rec)
    with pytest.raises(RuntimeError, match="no current batch"):
        eng.head(n5["cls_conv"], n5["cls_bias"])             # the current batch went with its record
    eng.import_pyramid(feats, SMALL)                         # ... and a fresh batch works as ever
    eng.head(n5["cls_conv"], n5["cls_bias"])
    assert all(d["scores"].numel() > 0 for d in eng.decode())
    live = eng.store_record()
    eng.close()                                              # releases live records
    assert live.closed


# ------------------------------------------------------------------------------------------------ 7: the model path, real backbone
def _equal_instances(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = g["instances"], w["instances"]
        assert len(w) > 0, f"{what}: image {i} has no detection"
        assert g.image_size == w.image_size and len(g) == len(w), f"{what}: image {i}"
        for f in ("scores", "pred_classes", "locations", "fpn_levels"):
            assert torch.equal(getattr(g, f), getattr(w, f)), f"{what}: image {i}: {f}"
        assert torch.equal(g.pred_boxes.tensor, w.pred_boxes.tensor), f"{what}: image {i}: pred_boxes"


def test_model_scores_record_inputs():
    from sylph_amd import synthetic as W
    from sylph_amd.runner import MetaFCOSRunner, create_cfg
    r = MetaFCOSRunner()
    cfg = create_cfg(r.get_default_cfg(), "sylph://COCO-Detection/Meta-FCOS/Meta-FCOS-finetune.yaml")
    model = r.build_model(cfg, dtype="bf16")
    model.load_state_dict(W.synthetic_state_dict(0, depth=50))
    model.eval()
    ims = [W.synthetic_images(1, 128, 160, seed=9)[0], W.synthetic_images(1, 100, 150, seed=10)[0]]
    batch = [{"image": ims[0], "height": 120, "width": 150, "image_id": 7, "file_name": "a.jpg"},
             {"image": ims[1], "height": 200, "width": 300, "image_id": 8, "file_name": "b.jpg"}]
    d0, d1, d2 = _code("n5"), _code("n5b"), _code("n20")
    kw = dict(run_type="meta_learn_test_instance")
    want = model(batch, class_code=d0, **kw)
    want_sets = model(batch, class_code_sets=[d0, d1, d2], **kw)
    want_mixed = model(batch, class_code=[d1, d2], **kw)
    records = model(batch, run_type="meta_learn_cache_query")
    assert len(records) == 1 and "image" not in records[0] and not any("image" in m for m in records[0]["inputs"])
    assert [m["image_id"] for m in records[0]["inputs"]] == [7, 8] and records[0]["inputs"][1]["file_name"] == "b.jpg"
    assert records[0]["record"].nbytes > 0 and records[0]["record"].batch[0] == 2
    model([{"image": ims[1], "height": 100, "width": 150}], class_code=d1, **kw)  # another batch in between
    _equal_instances(model(records, class_code=d0, **kw), want, "class_code")
    got_sets = model(records, class_code_sets=[d0, d1, d2], **kw)
    assert len(got_sets) == len(want_sets) == 3
    for g, (a, b) in enumerate(zip(got_sets, want_sets)):
        _equal_instances(a, b, f"class_code_sets, set {g}")
    _equal_instances(model(records, class_code=[d1, d2], **kw), want_mixed, "per-input class codes")
    with pytest.raises(ValueError, match="record"):
        model(records + [batch[0]], class_code=d0, **kw)
    records[0]["record"].close()
