"""Code-sets query step (sylph_fcos_head_codesets + sylph_decode_nms_codesets): every image of a batch is scored against G code sets
in one step -- the towers, box heads and cls GroupNorm statistics run once, the class-conditional conv and the decode per set.

The yardstick is the uniform step: `head(codes_g)` + `decode()` on the SAME engine and batch, which is itself pinned to the oracle
elsewhere.  For every (image, set) the code-sets step must return that run's rows bit for bit (`torch.equal` on every field of FIELDS,
the counts, and the exported logits in the set's columns); no tolerance is involved.  All cases but the model and runner ones drive
`Engine.import_pyramid` with distinct bf16-rounded randn pyramids (no backbone runs).

Codes: `synthetic_codes(n, seed, scale)` as listed in tests/test_mixed_episodes_gpu.py CODES.  Every case asserts its premises on what
the uniform runs return, so none can pass vacuously: every (image, set) has a detection, the two 5-way sets give different detections,
a 20- or 32-way set detects a class >= 8 (beyond the 8-float narrow logits pitch).  A decode that reports a status bit raises.

Column layout (csrc/api_internal.h Plan::cs.col0): the sets of up to 32 classes (bf16, cls GroupNorm) sit side by side, each at the
next multiple of 4, in blocks of 32 packed code rows, four blocks per launch of gn_logits_sets_kernel.  `_starts` restates that rule
for the premises "a set straddles a block boundary" / "a set ends at a block boundary"."""
import ctypes

import pytest
import torch

from test_head_sweeps_gpu import HW as HW_SWEEPS, LEVELS as LEVELS_SWEEPS, _premises, _pyramid as _sweeps_pyramid
from test_hip_parity import _cfg, _roienc_cfg
from test_mixed_episodes_gpu import FIELDS, SMALL, _code, _kernels, _new, _pairs, _pyramid, _same, _sd

pytestmark = pytest.mark.gpu

# kernels that belong to the class-conditional part of a head call (everything else in a profile: towers, box heads, statistics)
COND = ("gn_logits_kernel", "gn_logits_sets_kernel", "logits_scan_kernel", "gn_logits_episodes_kernel", "conv_igemm_kernel",
        "gn_apply_partials_kernel")


def _starts(ns):
    """first packed row of every set and the rows in use, all sets on the fused path: each set at the next multiple of 4"""
    out, col = [], 0
    for n in ns:
        out.append(col)
        col += (n + 3) // 4 * 4
    return out, col


def _uniform(eng, codes, export=True, **kw):
    """head(codes_g) + decode() [+ the logits export] per set -> ([g][i] detections, [g][level] logits)"""
    dets, logits = [], []
    for g, c in enumerate(codes):
        eng.head(c["cls_conv"], c["cls_bias"])
        d = eng.decode(**kw)
        for i, di in enumerate(d):
            assert di["scores"].numel() > 0, f"uniform run of set {g}: image {i} has no detection -- the comparison proves nothing"
        dets.append(d)
        logits.append([t.clone() for t in eng.export_head()[0]] if export else None)
    return dets, logits


def _check_sets(eng, codes, export=True, what="code sets", **kw):
    """The code-sets step against the uniform runs of its sets on the same engine and batch -> (kernel launches, got, want)."""
    want, want_lo = _uniform(eng, codes, export, **kw)
    k = _kernels(eng, lambda: eng.head_code_sets(_pairs(codes)))
    got = eng.decode_code_sets(**kw)
    assert len(got) == len(codes)
    for g, c in enumerate(codes):
        n = c["cls_conv"].shape[0]
        assert len(got[g]) == len(want[g])
        for i in range(len(want[g])):
            _same(got[g][i], want[g][i], f"{what}: set {g} ({n}-way), image {i}")
            assert int(got[g][i]["pred_classes"].max()) < n
    if export:
        lo = eng.export_head()[0]
        off, total = 0, sum(c["cls_conv"].shape[0] for c in codes)
        for g, c in enumerate(codes):
            n = c["cls_conv"].shape[0]
            for l in range(len(lo)):
                assert lo[l].shape[1] == total
                assert torch.equal(lo[l][:, off:off + n], want_lo[g][l]), f"{what}: set {g} level {l}: exported logits differ"
            off += n
    return k, got, want


def _assert_wide(dets, sets):
    for g in sets:
        top = max(int(d["pred_classes"].max()) for d in dets[g])
        assert top >= 8, f"set {g}: highest detected class {top}: columns >= 8 are not exercised"


def _assert_differ(a, b, what):
    assert a["scores"].numel() != b["scores"].numel() or not all(torch.equal(a[f], b[f]) for f in FIELDS), what


def _others(k):
    return {n: v for n, v in k.items() if n not in COND}


# ------------------------------------------------------------------------------------------------ 1: one block
def test_one_block_one_launch():
    """Sets of 5, 5 (other seed), 1 and 20 classes: 5 -> 8, 5 -> 8, 1 -> 4, 20 rows, 31 classes in one 32-row block plus 8 rows of a
    second one; one launch of the new kernel, none of gn_logits_kernel, the tower launches of ONE head call."""
    codes = [_code(k) for k in ("n5", "n5b", "n1", "n20")]
    assert sum(c["cls_conv"].shape[0] for c in codes) == 31
    eng = _new("bf16", _pyramid(3, SMALL), SMALL)
    uni = _kernels(eng, lambda: eng.head(codes[0]["cls_conv"], codes[0]["cls_bias"]))
    assert uni.get("gn_logits_kernel") == 1, uni
    k, got, want = _check_sets(eng, codes)
    print("uniform 5-way head:", uni, "\ncode-sets head:", k)
    assert k.get("gn_logits_sets_kernel") == 1 and "gn_logits_kernel" not in k and "logits_scan_kernel" not in k, k
    assert _others(k) == _others(uni) and k.get("conv_igemm_kernel") == uni.get("conv_igemm_kernel"), (k, uni)
    assert k.get("gn_apply_partials_kernel") == uni.get("gn_apply_partials_kernel"), (k, uni)
    _assert_wide(got, (3,))
    _assert_differ(want[0][1], want[1][1], "the two 5-way code sets give the same detections")
    eng.close()


# ------------------------------------------------------------------------------------------------ 2: straddling, several blocks
@pytest.mark.parametrize("names", [("n20", "n20", "n32", "n5", "n1"), ("n20", "n5", "n1", "n32", "n5b")],
                         ids=["20_20_32_5_1", "20_5_1_32_5"])
def test_sets_straddle_and_fill_blocks(names):
    """20, 20, 32, 5, 1 (78 classes, three blocks): the second set crosses row 32, the third row 64.  In that order no set ends on a
    block boundary (20, 40, 72, 77, 78 are no multiples of 32), so the second case places one: 20, 5, 1, 32, 5 puts the 1-way set in
    rows 28 .. 31 and the 32-way set in exactly block 1, rows 32 .. 63.  Both premises are asserted from the layout rule."""
    codes = [_code(k) for k in names]
    ns = [c["cls_conv"].shape[0] for c in codes]
    starts, rows = _starts(ns)
    crossing = [g for g, (s, n) in enumerate(zip(starts, ns)) if s // 32 != (s + n - 1) // 32]
    if names[1] == "n20":
        assert sum(ns) == 78 and crossing == [1, 2] and rows > 64, (starts, ns)
    else:
        assert [g for g, (s, n) in enumerate(zip(starts, ns)) if (s + n) % 32 == 0] == [3] and starts[3] == 32 and not crossing, (starts, ns)
    eng = _new("bf16", _pyramid(3, SMALL), SMALL)
    k, got, _ = _check_sets(eng, codes)
    assert k.get("gn_logits_sets_kernel") == 1 and "gn_logits_kernel" not in k, k
    _assert_wide(got, [g for g, n in enumerate(ns) if n >= 20])
    eng.close()


# ------------------------------------------------------------------------------------------------ 3: more than one pass
def test_five_32way_sets_two_passes():
    """160 packed rows: a pass of four blocks and a pass of one over the same tower output.  The sets are five different 32-way codes."""
    from sylph_amd import synthetic as W
    codes = [_code("n32")] + [{k: v.cuda() for k, v in W.synthetic_codes(32, seed=60 + s, scale=2.5).items()} for s in range(4)]
    eng = _new("bf16", _pyramid(3, SMALL), SMALL)
    k, got, want = _check_sets(eng, codes)
    assert k.get("gn_logits_sets_kernel") == 2 and "gn_logits_kernel" not in k, k
    _assert_wide(got, range(5))
    _assert_differ(want[0][0], want[1][0], "two 32-way code sets give the same detections")
    eng.close()


# ------------------------------------------------------------------------------------------------ 4: the cuts are per set
CUT_PRE, CUT_POST, CUT_THR = 10, 5, 0.02


def test_cuts_act_inside_one_set():
    """PRE_NMS_TOPK_TEST 10 per (image, level), POST_NMS_TOPK_TEST 5 per image, sets [a, a, b]: the duplicated set gives two identical
    slots, both equal to the uniform run.  A decode that ranked or suppressed across sets would cut the duplicate's candidates (equal
    scores, equal boxes, equal class indices) against each other."""
    cfg = _cfg(**{"MODEL.FCOS.PRE_NMS_TOPK_TEST": CUT_PRE, "MODEL.FCOS.POST_NMS_TOPK_TEST": CUT_POST, "MODEL.FCOS.INFERENCE_TH_TEST": CUT_THR})
    a, b = _code("n20"), _code("n5")
    eng = _new("bf16", _pyramid(3, SMALL), SMALL, cfg=cfg)
    # premises, on the uniform runs
    eng.head(a["cls_conv"], a["cls_bias"])
    uni = eng.decode()
    lo, _, ct, _ = eng.export_head()
    cand = torch.stack([((lo[l].sigmoid() > CUT_THR)).flatten(1).sum(1) for l in range(5)], 1).cpu()
    print("candidates per (image, level) of set a:", cand.tolist(), "detections per image:", [d["scores"].numel() for d in uni])
    assert int(cand.max()) > CUT_PRE, "no (image, level) has more candidates than PRE_NMS_TOPK_TEST"
    assert any(d["scores"].numel() == CUT_POST for d in uni), "no image returns exactly POST_NMS_TOPK_TEST rows"
    _, got, _ = _check_sets(eng, [a, a, b])
    for i in range(3):
        _same(got[1][i], got[0][i], f"image {i}: the two slots of the duplicated set")
    eng.close()


# ------------------------------------------------------------------------------------------------ 5: several sweeps
def test_three_sweeps_704_images():
    """The (96, 160) x B = 704 geometry of tests/test_head_sweeps_gpu.py: 4224 tiles over 2048 blocks, every wave of
    gn_logits_sets_kernel takes a second row group and blocks 0-127 a third, carrying the coefficient table.  G = 3, 42 classes."""
    from sylph_amd import synthetic as Wt
    from sylph_amd.engine import Engine
    codes = [_code(k) for k in ("n5", "n5b", "n32")]
    assert sum(c["cls_conv"].shape[0] for c in codes) == 42
    eng = Engine(_cfg(), dtype="bf16")
    eng.load_state_dict(Wt.head_state_dict(seed=1, num_classes=60))
    eng.import_pyramid(_sweeps_pyramid(704, LEVELS_SWEEPS, seed=11), HW_SWEEPS)
    _premises(eng, 704, HW_SWEEPS, LEVELS_SWEEPS, n_tiles=4224, sweeps=3)
    k, got, want = _check_sets(eng, codes, export=False)
    assert k.get("gn_logits_sets_kernel") == 1 and "gn_logits_kernel" not in k, k
    _assert_wide(got, (2,))
    _assert_differ(want[0][0], want[1][0], "the two 5-way code sets give the same detections")
    eng.close()


# ------------------------------------------------------------------------------------------------ 6: per-set routes
def _route_case(eng, codes, cold, what):
    """`cold` of the sets run conv_igemm (as the uniform head of their N does); the towers run once"""
    c5 = codes[0]
    uni = _kernels(eng, lambda: eng.head(c5["cls_conv"], c5["cls_bias"]))
    k, got, _ = _check_sets(eng, codes, what=what)
    print(what, "\nuniform 5-way head:", uni, "\ncode-sets head:", k)
    assert _others(k) == _others(uni), (k, uni)
    tower_igemm = uni.get("conv_igemm_kernel", 0) - (0 if uni.get("gn_logits_kernel") else 1)
    assert k.get("conv_igemm_kernel", 0) == tower_igemm + cold, (k, uni)
    assert "logits_scan_kernel" not in k and "gn_logits_kernel" not in k, k
    assert k.get("gn_apply_partials_kernel", 0) <= uni.get("gn_apply_partials_kernel", 0) + 1, (k, uni)  # the deferred apply: once
    return k, got


@pytest.mark.parametrize("dtype", ["f32", "f32s"])
def test_routes_fp32(dtype):
    eng = _new(dtype, _pyramid(3, SMALL), SMALL)
    k, got = _route_case(eng, [_code("n5"), _code("n20")], cold=2, what=dtype)
    assert "gn_logits_sets_kernel" not in k, k
    _assert_wide(got, (1,))
    eng.close()


def test_routes_bf16_5_and_60():
    """the 5-way set on the fused kernel (it reads the un-normalised tower output first), the 60-way set on the GroupNorm apply +
    conv_igemm that the uniform head's logits export runs"""
    eng = _new("bf16", _pyramid(3, SMALL), SMALL)
    k, got = _route_case(eng, [_code("n5"), _code("n60")], cold=1, what="bf16 5 + 60")
    assert k.get("gn_logits_sets_kernel") == 1, k
    _assert_wide(got, (1,))
    eng.close()


def test_routes_norm_none_bf16():
    cfg = _cfg(**{"MODEL.FCOS.NORM": "none"})
    eng = _new("bf16", _pyramid(3, SMALL), SMALL, sd=_sd(norm="none"), cfg=cfg)
    k, _ = _route_case(eng, [_code("n5"), _code("n20"), _code("n5b")], cold=3, what="NORM none")
    assert "gn_logits_sets_kernel" not in k, k
    eng.close()


def test_routes_roi_encoder():
    """CondConvBlock codes (two 256-channel chunks) fold into one 256-channel code per class on the host, per set"""
    from sylph_amd import synthetic as W
    sd = dict(_sd())
    sd.update(W.roi_encoder_state_dict(seed=4))
    eng = _new("bf16", _pyramid(3, SMALL), SMALL, sd=sd, cfg=_roienc_cfg())
    assert eng.is_roi_encoder
    _check_sets(eng, [_code("n5", c=512), _code("n20", c=512)], what="ROIEncoder")
    eng.close()


# ------------------------------------------------------------------------------------------------ 7: call sequences
def test_decode_twice_and_other_heads_around():
    codes = [_code(k) for k in ("n5", "n20", "n5b")]
    last = _code("n32")
    feats = _pyramid(3, SMALL)
    eng = _new("bf16", feats, SMALL)
    want, _ = _uniform(eng, codes, export=False)
    eng.head(last["cls_conv"], last["cls_bias"])
    want_last = eng.decode()
    # code-sets head -> decode -> decode again
    eng.head_code_sets(_pairs(codes))
    first = eng.decode_code_sets()
    again = eng.decode_code_sets()
    for g in range(3):
        for i in range(3):
            _same(first[g][i], want[g][i], f"first decode: set {g}, image {i}")
            _same(again[g][i], first[g][i], f"repeated decode: set {g}, image {i}")
    # code-sets head (not decoded) -> uniform head -> decode
    eng.head_code_sets(_pairs(codes))
    eng.head(last["cls_conv"], last["cls_bias"])
    got = eng.decode()
    for i in range(3):
        _same(got[i], want_last[i], f"uniform head after a code-sets head: image {i}")
    # head_episodes -> code-sets head -> decode
    eng.head_episodes(_pairs([codes[1], _code("n60")]), [0, 1, 0])  # (the 60-way episode leaves fused-scan candidates behind)
    eng.head_code_sets(_pairs(codes))
    got = eng.decode_code_sets()
    for g in range(3):
        for i in range(3):
            _same(got[g][i], want[g][i], f"after head_episodes: set {g}, image {i}")
    # ... and the uniform step after that decode is undisturbed
    eng.head(last["cls_conv"], last["cls_bias"])
    got = eng.decode()
    for i in range(3):
        _same(got[i], want_last[i], f"uniform step after a code-sets step: image {i}")
    eng.close()


def _decode_sets_raw(eng, G, B, max_out):
    """sylph_decode_nms_codesets through the C ABI -> (rc, counts [G * B], status)"""
    from sylph_amd.engine import _ptr
    S = max(G, 1) * B
    boxes, scores = torch.empty(S, max_out, 4, device="cuda"), torch.empty(S, max_out, device="cuda")
    ints = torch.empty(3, S, max_out, device="cuda", dtype=torch.int32)
    locs = torch.empty(S, max_out, 2, device="cuda")
    counts = torch.full((S + 1,), -7, device="cuda", dtype=torch.int32)
    rc = eng.L.sylph_decode_nms_codesets(eng._ctx, G, None, None, max_out, _ptr(boxes), _ptr(scores), _ptr(ints[0]), _ptr(ints[1]), _ptr(locs),
                                         _ptr(ints[2]), _ptr(counts), ctypes.c_void_p(counts.data_ptr() + 4 * S))
    torch.cuda.synchronize()
    c = counts.cpu().tolist()
    return rc, c[:S], c[S]


def test_wrong_decode_entry_wrong_G_and_truncation():
    codes = [_code(k) for k in ("n5", "n20")]
    eng = _new("bf16", _pyramid(2, SMALL), SMALL)
    want, _ = _uniform(eng, codes, export=False)
    # decode_code_sets after a uniform head
    with pytest.raises(RuntimeError, match="sylph_decode_nms"):
        eng.decode_code_sets()
    eng.head_code_sets(_pairs(codes))
    # decode after a code-sets head: refused before anything is written (the caller's buffers hold B slots, not G * B)
    with pytest.raises(RuntimeError, match="sylph_decode_nms_codesets"):
        eng.decode()
    # wrong G
    for G in (1, 3):
        rc, counts, _ = _decode_sets_raw(eng, G, 2, 64)
        assert rc != 0 and b"code sets" in eng.L.sylph_last_error()
        assert all(v == -7 for v in counts), "a refused call wrote counts"
    # a truncated max_out sets bit 1 and leaves nothing behind for the next decode
    most = max(d["scores"].numel() for ds in want for d in ds)
    assert most > 1
    rc, counts, status = _decode_sets_raw(eng, 2, 2, 1)
    assert rc == 0 and status & 2 and all(v == 1 for v in counts), (rc, counts, status)
    got = eng.decode_code_sets()
    for g in range(2):
        for i in range(2):
            _same(got[g][i], want[g][i], f"decode after a truncated one: set {g}, image {i}")
    with pytest.raises(RuntimeError, match="max_out"):
        eng.decode_code_sets(max_out=1)
    eng.close()


# ------------------------------------------------------------------------------------------------ 8: refusals
def test_refusals():
    from sylph_amd.engine import _iarr, _ptr
    c = _code("n5")
    eng = _new("bf16", _pyramid(2, SMALL), SMALL)
    with pytest.raises(ValueError, match="at least one code set"):
        eng.head_code_sets([])
    with pytest.raises(ValueError, match="empty"):
        eng.head_code_sets([(c["cls_conv"], c["cls_bias"]), (c["cls_conv"][:0], c["cls_bias"][:0])])
    with pytest.raises(ValueError, match="256"):
        eng.head_code_sets([(torch.zeros(5, 128, 1, 1, device="cuda"), c["cls_bias"])])
    with pytest.raises(ValueError, match="256"):
        eng.head_code_sets([(torch.zeros(5, 512, 1, 1, device="cuda"), c["cls_bias"])])  # (two chunks: a ROIEncoder model only)
    with pytest.raises(ValueError, match="every code set or for none"):
        eng.head_code_sets([(c["cls_conv"], c["cls_bias"]), (c["cls_conv"], None)])
    L, ctx = eng.L, eng._ctx
    w = c["cls_conv"].reshape(5, 256).contiguous()
    assert L.sylph_fcos_head_codesets(ctx, 0, _ptr(w), None, _iarr([5])) != 0 and b"G <= 0" in L.sylph_last_error()
    assert L.sylph_fcos_head_codesets(ctx, 1, _ptr(w), None, _iarr([0])) != 0 and b"empty" in L.sylph_last_error()
    assert L.sylph_fcos_head_codesets(ctx, 1, None, None, _iarr([5])) != 0 and b"NULL" in L.sylph_last_error()
    # none of them ran a head: nothing to decode
    with pytest.raises(RuntimeError, match="must be called first"):
        eng.decode()
    eng.close()


def test_3x3_codes_are_refused_by_name():
    from sylph_amd.engine import _iarr, _ptr
    cfg = _cfg(**{"MODEL.META_LEARN.CODE_GENERATOR.CLS_LAYER": ["", "", 3]})
    eng = _new("bf16", _pyramid(2, SMALL), SMALL, cfg=cfg)
    assert eng.code_ksize == 3
    w, b = torch.zeros(2, 2304, device="cuda"), torch.zeros(2, device="cuda")
    rc = eng.L.sylph_fcos_head_codesets(eng._ctx, 1, _ptr(w), _ptr(b), _iarr([2]))
    assert rc != 0 and b"CLS_LAYER" in eng.L.sylph_last_error()
    with pytest.raises(NotImplementedError, match="CLS_LAYER"):
        eng.head_code_sets([(torch.zeros(2, 256, 3, 3, device="cuda"), b)])
    eng.close()


# ------------------------------------------------------------------------------------------------ 9: the model API
@pytest.fixture(scope="module")
def model():
    from sylph_amd import synthetic as W
    from sylph_amd.runner import MetaFCOSRunner, create_cfg
    r = MetaFCOSRunner()
    cfg = create_cfg(r.get_default_cfg(), "sylph://COCO-Detection/Meta-FCOS/Meta-FCOS-finetune.yaml", ["TEST.REPEAT_TEST", 3])
    m = r.build_model(cfg, dtype="bf16")
    m.load_state_dict(W.synthetic_state_dict(0, depth=50))
    m.eval()
    return r, cfg, m


def test_model_class_code_sets(model):
    from sylph_amd import synthetic as W
    _, _, m = model
    batch = [{"image": im, "height": 120, "width": 150} for im in W.synthetic_images(2, 128, 160, seed=9)]
    sets = [_code("n5"), _code("n5b"), _code("n20")]
    kw = dict(run_type="meta_learn_test_instance")
    got = m(batch, class_code_sets=sets, **kw)
    assert len(got) == 3 and all(len(g) == 2 for g in got)
    for g, d in enumerate(sets):
        want = m(batch, class_code=d, **kw)
        for i in range(2):
            a, w = got[g][i]["instances"], want[i]["instances"]
            assert len(w) > 0, f"uniform call {g}: image {i} has no detection"
            assert a.image_size == w.image_size == (120, 150) and len(a) == len(w)
            for f in ("scores", "pred_classes", "locations", "fpn_levels"):
                assert torch.equal(getattr(a, f), getattr(w, f)), f"set {g}, image {i}: {f}"
            assert torch.equal(a.pred_boxes.tensor, w.pred_boxes.tensor), f"set {g}, image {i}: pred_boxes"
    a, b = got[0][0]["instances"], got[1][0]["instances"]
    assert len(a) != len(b) or not torch.equal(a.scores, b.scores), "image 0 gets the same detections under two code sets"
    with pytest.raises(ValueError, match="both"):
        m(batch, class_code=sets[0], class_code_sets=sets, **kw)
    with pytest.raises(ValueError):
        m(batch, class_code_sets=[], **kw)


# ------------------------------------------------------------------------------------------------ 10: the runner
class _Record:
    """keeps every image's detections; its result is a function of all of them"""

    def reset(self):
        self.rows = []

    def process(self, inputs, outputs):
        for x, o in zip(inputs, outputs):
            i = o["instances"]
            self.rows.append((x["image_id"], i.pred_boxes.tensor.cpu(), i.scores.cpu(), i.pred_classes.cpu()))

    def evaluate(self):
        n = sum(r[2].numel() for r in self.rows)
        s = float(sum(r[2].double().sum() for r in self.rows))
        return {"bbox": {"AP": s, "AP50": float(n), "APr": float(sum(int(r[3].sum()) for r in self.rows))}}


def test_runner_fuse_repeats(model, tmp_path):
    """REPEAT_TEST = 3 over synthetic loaders: fuse_repeats=True returns the results dict of the default loop -- seed entries, means,
    _avg / _std -- from ONE backbone pass per query batch instead of three."""
    from sylph_amd.data import SyntheticQueryLoader, SyntheticSupportSetLoader
    from sylph_amd.runner import MetaFCOSRunner
    _, cfg, m = model
    NQ, BS = 3, 2

    class R(MetaFCOSRunner):
        evs = []

        def build_episodic_learning_detection_test_support_set_loader(self, cfg, name, seed=0):
            return SyntheticSupportSetLoader(3, 1, 128, 160, seed=20 + seed)

        def build_episodic_learning_detection_test_query_loader(self, cfg, name):
            return SyntheticQueryLoader(NQ, 120, 152, batch_size=BS, seed=4)

        def get_evaluator(self, cfg, name, output_folder=None):
            R.evs.append(_Record())
            return R.evs[-1]

    cfg = cfg.clone()
    cfg.DATASETS.TEST = ("synthetic_meta_val_novel",)
    cfg.OUTPUT_DIR = str(tmp_path / "output")
    cfg.MODEL.META_LEARN.USE_ALL_GTS_IN_BASE_CLASSES = False
    assert int(cfg.TEST.REPEAT_TEST) == 3
    calls = {"n": 0}
    run_backbone = m._run_backbone

    def counting(batched_inputs):
        calls["n"] += 1
        return run_backbone(batched_inputs)

    m._run_backbone = counting
    try:
        r = R()
        want = r._do_test_meta_learning(cfg, m)
        n_unfused, evs_unfused = calls["n"], R.evs
        calls["n"], R.evs = 0, []
        got = r._do_test_meta_learning(cfg, m, fuse_repeats=True)
        n_fused, evs_fused = calls["n"], R.evs
    finally:
        del m._run_backbone
    batches = -(-NQ // BS)
    assert n_unfused == 3 * batches and n_fused == batches, (n_unfused, n_fused)
    assert list(got) == list(want) == ["default", "seed0", "seed1", "seed2"]
    assert got == want, (got, want)
    name = "synthetic_meta_val_novel"
    assert "AP_std" in got["default"][name]["bbox"] and got["default"][name]["bbox"]["AP_std"] > 0.0, "the seeds' code sets give equal results"
    assert all(got[f"seed{s}"][name]["bbox"]["AP50"] > 0 for s in range(3)), "a seed has no detection"
    for s in range(3):  # evaluator s saw what the unfused loop showed it, row for row
        a, b = evs_fused[s].rows, evs_unfused[s].rows
        assert [x[0] for x in a] == [x[0] for x in b] == list(range(NQ))
        for x, y in zip(a, b):
            assert all(torch.equal(p, q) for p, q in zip(x[1:], y[1:])), f"seed {s}, image {x[0]}"


# ------------------------------------------------------------------------------------------------ 11: the grow paths
def _grow_steps():
    """The sequence of test_buffers_grow_in_place_and_settle: (name, step), step(eng) -> the detections as a list of per-image lists"""
    c = {k: _code(k) for k in ("n5", "n5b", "n20", "n60")}

    def head(k):
        def run(eng):
            eng.head(c[k]["cls_conv"], c[k]["cls_bias"])
            return [eng.decode()]
        return run

    def sets(*ks):
        def run(eng):
            eng.head_code_sets(_pairs([c[k] for k in ks]))
            return eng.decode_code_sets()
        return run

    def episodes(eng):
        eng.head_episodes(_pairs([c["n5"], c["n60"]]), [0, 1])
        return [eng.decode()]

    return [("1 head(n5)", head("n5")), ("2 sets[n5]", sets("n5")), ("3 sets[n5, n20, n5b]", sets("n5", "n20", "n5b")),
            ("4 sets[n20, n60]", sets("n20", "n60")), ("5 episodes[n5, n60]", episodes), ("6 head(n60)", head("n60")),
            ("7 sets[n5]", sets("n5")), ("8 head(n5)", head("n5"))]


def _same_step(got, want, what):
    assert len(got) == len(want), what
    for g, (a, b) in enumerate(zip(got, want)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{what}: slot {g}, image {i}")


def test_buffers_grow_in_place_and_settle():
    """One bf16 engine, two images, every head in turn with growing and shrinking requests: the packed code / bias tables, the logits,
    the decode slots and the candidate buffers of the B-slot and the G * B-slot decodes grow step by step, a 60-way fused scan leaves
    candidates between two of the growths, and smaller requests reuse what is there.  Every step returns what a fresh engine that runs
    only that step returns; a second pass over the sequence returns the same and allocates nothing."""
    B = 2
    feats = _pyramid(B, SMALL)
    steps = _grow_steps()
    want = {}
    for name, step in steps:
        fresh = _new("bf16", feats, SMALL)
        want[name] = step(fresh)
        fresh.close()
        assert all(d["scores"].numel() > 0 for slot in want[name] for d in slot), f"{name}: an image has no detection on a fresh engine"
    _same_step(want["8 head(n5)"], want["1 head(n5)"], "fresh engines: step 8 against step 1")
    eng = _new("bf16", feats, SMALL)
    bytes_after = []
    for rep in range(2):
        got = {}
        for name, step in steps:
            before = eng.device_bytes()
            got[name] = step(eng)
            grew = eng.device_bytes() - before
            print(f"pass {rep}, step {name}: device bytes {before} {grew:+d}")
            _same_step(got[name], want[name], f"pass {rep}, step {name}")
            if rep == 0 and name[0] in "346":
                assert grew > 0, f"step {name} allocated nothing: the sequence exercises no growth there"
            if rep == 1:
                assert grew == 0, f"second pass, step {name}: {grew} bytes allocated in the steady state"
        _same_step(got["8 head(n5)"], got["1 head(n5)"], f"pass {rep}: step 8 against step 1")
        bytes_after.append(eng.device_bytes())
    assert bytes_after[1] == bytes_after[0], bytes_after
    eng.close()
