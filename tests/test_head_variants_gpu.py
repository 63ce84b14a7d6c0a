"""The FCOS head's tower variants under every head entry (csrc/api_head.hip: build_head and the entries that consume what it left).

build_head assembles the query head from independent switches -- MODEL.FCOS.NORM, NUM_SHARE_CONVS, NUM_CLS_CONVS / NUM_BOX_CONVS,
USE_DEFORMABLE, the storage dtype -- and every head entry reads what that build left behind (Plan::cls_feat, cls_coef, cls_apply, cls_gn).
Each switch and each entry is pinned elsewhere on the default head; this file runs the cross terms of tests/head_variants.py::VARIANTS,
all on one pyramid of 128 x 160 (levels down to 2 x 3 and 1 x 2, three ragged images):

  premise   one head call launches conv_deform_kernel once per deformable tower of the table (2 / 1 / 0);
  a  f32, f32s: export_head within 1e-3 x max(1, max|want|) of the float64 restatement (tests/deform_ref.py) for 5 and 40 classes, and the
     decode of the engine's own head picks the candidates the decode of the imported restatement picks;
  b  bf16: the deformable layer of every observable tower within the bars of tests/test_deform_gpu.py::_pin_layer, with the variant's
     random offsets and with exact constant offsets that leave every map on all four sides;
  c  bf16, tolerance-free identities per entry: fused many-way scan == unfused route == the oracle decoder; mixed episodes == uniform
     heads; code sets == one head per set; pretrained head == head(cls_logits); a stored record scored 5-way, 40-way, pretrained and
     exported == the fresh batch; 3x3 codes against the restatement and under SYLPH_GN_COND3X3;
  d  bf16: export_head within 6e-2 x max(1, max|want|) of the restatement (a wrong table that every entry shares).

Every compared decode first asserts a detection on every image.  Measured figures are printed before they are asserted; on an MI355X
(worst over the 5- and 40-way codes; layer pin in bf16 ulps, random / exact offsets):

  variant           f32      f32s     bf16     layer pin        bars: 1e-3, 1e-3, 6e-2, 4 / 1 ulp
  gn_d              9.5e-6   4.3e-5   3.4e-2   2.00 / 1.00
  none_d            7.5e-6   4.4e-5   2.2e-2   2.00 / 1.00
  gn_share_d        6.0e-6   4.3e-5   2.7e-2   1.50 / 1.00
  gn_c1b3_d         8.0e-6   3.6e-5   2.3e-2   2.00 / 1.00
  gn_c0b2_d         5.4e-6   2.6e-5   2.1e-2   1.00 / 1.00
  none_share_c1_d   6.6e-6   4.6e-5   2.8e-2   3.00 / 1.00
  gn_share          3.9e-6   2.4e-5   1.5e-2   (no deformable layer)
  none_share        2.9e-6   2.4e-5   1.2e-2   (no deformable layer)
  3x3 codes: gn_d 9.5e-6 (f32), 3.4e-2 (bf16); none_d 7.5e-6, 2.2e-2

One variant x entry missed its identity: under SYLPH_GN_COND3X3=1 the scores of gn_d differ from the default route's in the last fp32
bit (gn_cond3x3_kernel adds nine per-tap accumulators, conv_igemm runs one).  That cannot be made equal in the kernel as it is designed,
so the library now refuses the fused 3x3 route for deformable towers, and test_3x3_codes_under_the_fused_knob[gn_d] tests the refusal."""
import numpy as np
import pytest
import torch

from tests import head_variants as HV
from test_deform_gpu import _pin_layer
from test_mixed_episodes_gpu import _check_mixed, _kernels, _pairs, _same
from test_records_gpu import _assert_detects, _equal_runs, _pretrained, _uniform

pytestmark = pytest.mark.gpu

ALL = list(HV.VARIANTS)
DEFORMABLE = [v for v in ALL if HV.VARIANTS[v][4]]
K3 = "MODEL.META_LEARN.CODE_GENERATOR.CLS_LAYER"
KNOB = "SYLPH_GN_COND3X3"  # read at every head call


def _engine(v, dtype, taps=False, sd=None, fs=None, **over):
    from sylph_amd.engine import Engine
    eng = Engine(HV.cfg(v, **over), dtype=dtype)
    eng.load_state_dict(sd if sd is not None else HV.state_dict(v))
    if taps:
        eng.set_debug_taps(True)
    eng.import_pyramid(fs if fs is not None else HV.feats(), HV.HW, HV.SIZES)
    assert eng.level_shapes(*HV.HW) == HV.LEVELS
    return eng


def _cuda(c):
    return {k: t.cuda() for k, t in c.items()}


def _detects(dets, what):
    for i, d in enumerate(dets):
        assert d["scores"].numel() > 0, f"{what}: image {i} has no detection -- the comparison proves nothing"


@pytest.fixture(scope="module", params=ALL)
def bf16(request):
    """one bf16 engine per variant, as a serving process builds it (no debug taps), shared by the entry identities"""
    eng = _engine(request.param, "bf16")
    yield request.param, eng
    eng.close()


# ------------------------------------------------------------------------------------------------ premise
def test_table_builds_the_deformable_towers_it_names(bf16):
    """a variant that silently built a plain conv (or a deformable one where none is configured) fails here"""
    v, eng = bf16
    c = _cuda(HV.codes("n5"))
    eng.import_pyramid(HV.feats(), HV.HW, HV.SIZES)
    k = _kernels(eng, lambda: eng.head(c["cls_conv"], c["cls_bias"]))
    print(v, k)
    assert k.get("conv_deform_kernel", 0) == HV.deform_towers(v), (v, k)
    assert [HV.deform_towers(x) for x in ALL] == [2, 2, 2, 2, 1, 2, 0, 0]


# ------------------------------------------------------------------------------------------------ a: fp32 storage
@pytest.mark.parametrize("dtype", ["f32", "f32s"])
@pytest.mark.parametrize("v", ALL)
def test_fp32_head_matches_restatement_and_decoder(v, dtype):
    for name in ("n5", "n40"):
        thr, half, sep = HV.threshold(v, name)
        eng = _engine(v, dtype, **{"MODEL.FCOS.INFERENCE_TH_TEST": thr})
        c, want = HV.codes(name), HV.reference(v, name)
        eng.head(c["cls_conv"], c["cls_bias"])
        got = eng.export_head()
        worst = HV.worst_rel(got, want)
        print(f"{v} {dtype} {name}: worst head difference {worst:.2e} (logits alone {HV.worst_rel(got[:1], want[:1]):.2e}; "
              f"threshold {thr:.4f}, nearest class probability {half:.1e}, detection scores {sep:.1e} apart)")
        assert worst <= 1e-3, (v, dtype, name, worst)
        mine = eng.decode()
        eng.import_head(*[[t.float() for t in ts] for ts in want])
        ref = eng.decode()
        _detects(mine, f"{v} {dtype} {name}: the engine's own head")
        _detects(ref, f"{v} {dtype} {name}: the imported restatement")
        for i, (a, b) in enumerate(zip(mine, ref)):
            ca, cb = a["cand_index"].cpu().tolist(), b["cand_index"].cpu().tolist()
            print(f"{v} {dtype} {name}: image {i}: {len(ca)} / {len(cb)} detections")
            assert ca == cb, (f"{v} {dtype} {name}: image {i} picks other candidates: only mine {sorted(set(ca) - set(cb))}, only the "
                              f"restatement's {sorted(set(cb) - set(ca))}, same set in another order: {sorted(ca) == sorted(cb)}")
        eng.close()


# ------------------------------------------------------------------------------------------------ b: the deformable layer, bf16
def _pin(v, sd, what, exact):
    norm, share, nc, nb, _ = HV.VARIANTS[v]
    fs = HV.feats()
    eng = _engine(v, "bf16", taps=True, sd=sd, fs=fs)
    c = _cuda(HV.codes("n5"))
    eng.head(c["cls_conv"], c["cls_bias"])
    # a one-layer tower behind a shared tower reads the shared tower's output, which export_tower does not expose
    skip = tuple(t for t, n in ((0, nc), (1, nb)) if n == 1 and share > 0)
    assert skip == ((0,) if v == "none_share_c1_d" else ()), (v, skip)
    worst = _pin_layer(eng, sd, what, exact_offsets=exact, convs=(nc, nb), norm=norm, pyramid=fs, skip=skip)
    print(f"{what}: worst {worst:.2f} bf16 ulp")
    eng.close()


@pytest.mark.parametrize("v", DEFORMABLE)
def test_deformable_layer_pinned_bf16(v):
    _pin(v, HV.state_dict(v), f"{v} random offsets", exact=False)


@pytest.mark.parametrize("v", DEFORMABLE)
def test_deformable_layer_borders_bf16(v):
    """constant offsets of up to +-9 px per tap, fractional ones among them: taps leave the 2 x 3 and the 1 x 2 map (and the 4 x 5 one)
    entirely and every larger map on all four sides; zero offset-conv weights make the offsets exact on both sides: 1 ulp"""
    sd = HV.state_dict(v)
    shifts = [(-9.0, 0.3), (9.0, -0.6), (0.4, -9.0), (-0.7, 9.0), (-9.0, -9.0), (9.0, 9.0), (3.5, -2.25), (-1.0, 0.0), (0.0, 7.0)]
    for tower in ("cls_tower", "bbox_tower"):
        pre = HV.last_layer_key(v, tower)
        if pre is None:
            continue
        sd[f"{pre}.offset.weight"].zero_()
        for j, (dy, dx) in enumerate(shifts):
            sd[f"{pre}.offset.bias"][2 * j] = dy
            sd[f"{pre}.offset.bias"][2 * j + 1] = dx
    _pin(v, sd, f"{v} borders", exact=True)


# ------------------------------------------------------------------------------------------------ c: the head entries, bf16
def _cond_kernel_premise(v, eng, c, k):
    """which class-conditional kernel a 40-way head must have run (api_head.hip: head_kind): the fused conv + scan where the build left a
    deferred cls GroupNorm (GroupNorm towers with a cls tower), otherwise ONE conv_igemm launch on top of the towers' own"""
    norm, share, nc, nb, _ = HV.VARIANTS[v]
    if norm == "GN" and nc > 0:
        assert k.get("logits_scan_kernel") == 1 and "gn_logits_kernel" not in k and "gn_apply_partials_kernel" not in k, (v, k)
        return
    towers = _kernels(eng, eng.towers)
    assert not {"logits_scan_kernel", "gn_logits_kernel", "gn_apply_partials_kernel"} & set(k), (v, k)
    assert k.get("conv_igemm_kernel", 0) == towers.get("conv_igemm_kernel", 0) + 1, (v, k, towers)


def test_many_way_scan_equals_unfused_and_oracle(bf16):
    v, eng = bf16
    c = _cuda(HV.codes("n40"))
    eng.import_pyramid(HV.feats(), HV.HW, HV.SIZES)
    k = _kernels(eng, lambda: eng.head(c["cls_conv"], c["cls_bias"]))
    fused = eng.decode()
    lo, rg, ct, io = eng.export_head()  # (after a scan: the unfused conv on the same tower output)
    eng.import_head(lo, rg, ct, io)     # ... whose logits go through decode_scan_kernel
    unfused = eng.decode()
    _detects(fused, f"{v}: 40-way head")
    _detects(unfused, f"{v}: decode of the exported logits")
    want = HV.oracle_detections((lo, rg, ct, io), 0.05)
    for i, (f, u, w) in enumerate(zip(fused, unfused, want)):
        _same(f, u, f"{v}: image {i}, head + decode against export -> import -> decode")
        assert f["scores"].numel() == w["scores"].numel(), (v, i)
        np.testing.assert_array_equal(f["pred_classes"].cpu().numpy(), w["pred_classes"].numpy())
        np.testing.assert_array_equal(f["locations"].cpu().numpy(), w["locations"].numpy())
        np.testing.assert_allclose(f["scores"].cpu().numpy(), w["scores"].numpy(), atol=1e-5)
    eng.import_pyramid(HV.feats(), HV.HW, HV.SIZES)
    _cond_kernel_premise(v, eng, c, k)


def test_mixed_episodes_equal_uniform_heads(bf16):
    v, eng = bf16
    eng.import_pyramid(HV.feats(), HV.HW, HV.SIZES)
    codes = [_cuda(HV.codes(n)) for n in ("n5", "n20", "n40")]
    _check_mixed(eng, codes, [1, 2, 0], what=f"{v}: 5-, 20- and 40-way episodes")  # (asserts a detection per image on the uniform runs)


def test_code_sets_equal_one_head_per_set(bf16):
    v, eng = bf16
    eng.import_pyramid(HV.feats(), HV.HW, HV.SIZES)
    codes = [_cuda(HV.codes(n)) for n in ("n5", "n20")]
    eng.head_code_sets(_pairs(codes))
    got = eng.decode_code_sets()
    assert len(got) == 2
    for g, c in enumerate(codes):
        eng.head(c["cls_conv"], c["cls_bias"])
        want = eng.decode()
        _detects(want, f"{v}: uniform head of code set {g}")
        for i in range(3):
            _same(got[g][i], want[i], f"{v}: code set {g}, image {i}")


def test_pretrained_head_equals_head_on_cls_logits(bf16):
    v, eng = bf16
    sd = HV.state_dict(v)
    w, b = sd[f"{HV.P}.cls_logits.weight"].cuda(), sd[f"{HV.P}.cls_logits.bias"].cuda()
    eng.import_pyramid(HV.feats(), HV.HW, HV.SIZES)
    assert eng.head_pretrained() == 60
    got = eng.decode()
    eng.head(w, b)
    want = eng.decode()
    _detects(want, f"{v}: head(cls_logits)")
    for i in range(3):
        _same(got[i], want[i], f"{v}: pretrained head, image {i}")


def test_record_scored_like_the_fresh_batch(bf16):
    """towers -> store; the plan's buffers overwritten by another batch; the record scored 5-way (streamed in place where the build left a
    deferred GroupNorm), 40-way, by the pretrained head (restore_record: features, coefficient and partial tables copied back), and its
    logits exported after the 40-way scan"""
    v, eng = bf16
    fs, other = HV.feats(), HV.feats(seed=34)
    runs = [("5-way", _uniform(_cuda(HV.codes("n5")))), ("40-way", _uniform(_cuda(HV.codes("n40")), export=False)),
            ("pretrained", _pretrained)]
    c40 = _cuda(HV.codes("n40"))
    eng.import_pyramid(fs, HV.HW, HV.SIZES)
    want = []
    for what, run in runs:
        want.append(run(eng))
        _assert_detects(want[-1][0], f"{v}: fresh {what}")
    eng.head(c40["cls_conv"], c40["cls_bias"])
    want_export = eng.export_head()
    eng.import_pyramid(fs, HV.HW, HV.SIZES)
    eng.towers()
    rec = eng.store_record()
    eng.import_pyramid(other, HV.HW, HV.SIZES)
    eng.towers()
    eng.load_record(rec)
    for (what, run), w in zip(runs, want):
        _equal_runs(run(eng), w, f"{v}: record, {what}")
    eng.head(c40["cls_conv"], c40["cls_bias"])
    got_export = eng.export_head()
    for t, name in enumerate(("logits", "reg", "ctr", "iou")):
        for l in range(5):
            assert torch.equal(got_export[t][l], want_export[t][l]), f"{v}: record, export after the 40-way head: {name}, level {l}"
    assert not torch.equal(fs[0], other[0])
    rec.close()


@pytest.mark.parametrize("v", ["gn_d", "none_d"])
@pytest.mark.parametrize("dtype,bar", [("f32", 1e-3), ("bf16", 6e-2)])
def test_3x3_codes_match_restatement(v, dtype, bar, monkeypatch):
    """the default route of a 3x3 class code (deferred GroupNorm apply + conv_igemm; conv_igemm alone without a tower norm)"""
    monkeypatch.delenv(KNOB, raising=False)
    c, want = HV.codes3(), HV.reference(v, "k3")
    eng = _engine(v, dtype, **{K3: ["", "", 3]})
    k = _kernels(eng, lambda: eng.head(c["cls_conv"], c["cls_bias"]))
    assert "gn_cond3x3_kernel" not in k and k.get("conv_deform_kernel") == 2, k
    got = eng.export_head()
    worst = HV.worst_rel(got, want)
    print(f"{v} 3x3 codes {dtype}: worst head difference {worst:.2e} (logits alone {HV.worst_rel(got[:1], want[:1]):.2e})")
    assert worst <= bar, (v, dtype, worst)
    _detects(eng.decode(), f"{v} {dtype}: 3x3 codes")
    eng.close()


@pytest.mark.parametrize("v", ["gn_d", "none_d"])
def test_3x3_codes_under_the_fused_knob(v, monkeypatch):
    """SYLPH_GN_COND3X3=1 against the default route on one engine, every field with torch.equal -- wherever a head runs under the knob.

    none_d has no GroupNorm to fuse: the knob changes nothing and the detections are the default route's, bit for bit.
    gn_d: gn_cond3x3_kernel picks the default route's detections (counts, classes, levels, locations and candidate ordinals were equal
    on all three images, 100 / 99 / 99 detections) but keeps one fp32 accumulator per tap and adds the nine in a fixed order
    (csrc/head_fused.hip), conv_igemm one accumulator over K = 2 304: scores came out one fp32 ulp apart (largest difference
    2.98e-07 / 2.98e-07 / 3.58e-07 on images 0 / 1 / 2).  The identity cannot hold for that kernel, so sylph_fcos_head refuses the
    combination before it launches anything (config_from_cfg too: tests/test_head_variants_cpu.py); the refusal is what is tested,
    and that it leaves the engine serving the default route unchanged."""
    c = HV.codes3()
    eng = _engine(v, "bf16", **{K3: ["", "", 3]})
    monkeypatch.delenv(KNOB, raising=False)
    eng.head(c["cls_conv"], c["cls_bias"])
    default = eng.decode()
    _detects(default, f"{v}: 3x3 codes, default route")
    monkeypatch.setenv(KNOB, "1")
    if v == "gn_d":
        with pytest.raises(RuntimeError, match="SYLPH_GN_COND3X3=1 with MODEL.FCOS.USE_DEFORMABLE"):
            eng.head(c["cls_conv"], c["cls_bias"])
        with pytest.raises(RuntimeError, match="sylph_fcos_head must be called first"):
            eng.decode()  # the refused call left nothing to decode
        monkeypatch.delenv(KNOB)
    k = _kernels(eng, lambda: eng.head(c["cls_conv"], c["cls_bias"]))
    assert "gn_cond3x3_kernel" not in k, (v, k)  # (NORM "none": no deferred GroupNorm to fuse, whatever the knob says)
    again = eng.decode()
    eng.close()
    for f in ("pred_classes", "fpn_levels", "locations", "cand_index", "scores", "pred_boxes"):
        for i in range(3):
            assert again[i]["scores"].numel() == default[i]["scores"].numel(), (v, i)
            assert torch.equal(again[i][f], default[i][f]), f"{v}: 3x3 codes, image {i}: {f} differs"


# ------------------------------------------------------------------------------------------------ d: bf16 against float64
def test_bf16_head_close_to_restatement(bf16):
    v, eng = bf16
    for name in ("n5", "n40"):
        c = _cuda(HV.codes(name))
        eng.import_pyramid(HV.feats(), HV.HW, HV.SIZES)
        eng.head(c["cls_conv"], c["cls_bias"])
        got, want = eng.export_head(), HV.reference(v, name)
        worst = HV.worst_rel(got, want)
        print(f"{v} bf16 {name}: worst head difference {worst:.2e} (logits alone {HV.worst_rel(got[:1], want[:1]):.2e})")
        assert worst <= 6e-2, (v, name, worst)
