"""Class codes from ROI lists (sylph_codegen_rois / sylph_roi_align_rois): many boxes per image, ragged shot counts.

The definition under test: segment j of a ROI list is ONE reference call on a support set whose shot i is the pyramid of the
segment's i-th ROI's image with that ROI's box.  Hence the two comparisons every test here is made of:
  * the DUPLICATE BATCH: import_pyramid([f[roi_image] for f in feats]) holds image roi_image[r] as its image r, so the existing
    one-box-per-image entry points run the same kernels at the same launch sizes on identical operands: torch.equal, no tolerance.
  * the PARENT'S BITS for the one-box-per-image entry points, which run the same pass with roi_image[r] = r (g12_parent_support.npz).
  * the per-segment restatements: tests/bf16_ulps.py codegen_tail_f64 on the exported per-ROI maps (its own fp32 summation bound), the
    mean of the exported tokens (1e-4 of max(1, max |want|), assert_f32), a lone Engine.codegen call per segment (the same 1e-4: a
    small lone call may take another conv route, so no bit claim) and the fp32 oracle through tests/support_rois_ref.py (1e-3, the
    tolerance tests/test_hip_parity.py uses for fp32 codes).
Pyramids go in through Engine.import_pyramid at 64 x 96 as in tests/test_support_bf16_pinned_gpu.py, whose helpers and route names
are used here; R = 60 and R = 183 sit on the two sides of its conv_hpipe threshold (183: the odd pad patch, 64 x 128 cls-conv tiles)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from bf16_ulps import assert_f32, assert_tail, assert_ulps, bf16_rne, codegen_tail_f64
from independent_refs import level_of_box, roi_pool_separable_f64
from support_rois_ref import segment_codes
from test_support_bf16_pinned_gpu import AUX, _box_kinds, _box_sets, _cfg, _engine, _expected_routes, _pyramid, _routing_overrides, _state_dict

pytestmark = pytest.mark.gpu

H, W = 64, 96
F32_REL = 1e-4  # assert_f32's bound for fp32 sums over K = 2304 products


def _roi_images(R, B, unused, heavy, seed):
    """R image indices in [0, B): `unused` never appears, `heavy` exactly 7 times, the rest share the remainder; scattered order."""
    others = [b for b in range(B) if b not in (unused, heavy)]
    v = [heavy] * 7 + [others[i % len(others)] for i in range(R - 7)]
    g = torch.Generator().manual_seed(seed)
    v = [v[i] for i in torch.randperm(R, generator=g).tolist()]
    assert any(a > b for a, b in zip(v, v[1:])) and any(a < b for a, b in zip(v, v[1:])), "not scattered"
    assert v.count(heavy) == 7 and v.count(unused) == 0 and set(v) == set(others) | {heavy}
    return v


def _dup(feats, roi_image):
    idx = torch.tensor(roi_image)
    return [f[idx] for f in feats]


def _stages(kind):
    if kind == "roienc":
        return ([("roi", 0), ("mscam", 0), ("cls_tokens", 0)] + [(s, i) for s in ("gn_y", "gn_coef", "layer_out") for i in range(3)]
                + [("tokens", i) for i in range(3)])
    return [("roi", 0), ("conv_out", 0), ("conv_out", 1)] + [(s, i) for s in ("gn_y", "gn_coef", "layer_out") for i in range(2)]


# ------------------------------------------------------------------------------------------------ 1. duplicate batch, bit for bit
@pytest.mark.parametrize("R,shots", [(60, 5), (183, 3)])
@pytest.mark.parametrize("kind", ["codegen", "weighted", "roienc"])
@pytest.mark.parametrize("dtype", ["f32", "f32s", "bf16"])
def test_roi_list_equals_duplicate_batch(dtype, kind, R, shots):
    B = 8
    feats = _pyramid(B, H, W, seed=B)
    roi_image = _roi_images(R, B, unused=5, heavy=2, seed=R)
    boxes = _box_sets(R, H, W, seed=100 + R)[0]
    seg_len = [shots] * (R // shots)
    eng = _engine(kind, dtype=dtype)
    eng.import_pyramid(feats, (H, W))
    codes = eng.codegen_rois(boxes, roi_image, seg_len).clone()
    routes = eng.conv_routes()
    assert tuple(codes.shape) == (R // shots, 257)
    wn = eng.codegen_weight_norm(len(seg_len)).clone() if kind == "weighted" else None
    got = {s: eng.export_support(*s).clone() for s in _stages(kind)}
    ctx = eng.export_support("context").clone() if kind == "roienc" else None

    eng.import_pyramid(_dup(feats, roi_image), (H, W))
    want = eng.codegen_classes(boxes, shots).clone()
    routes_dup = eng.conv_routes()
    print(f"{dtype} {kind} R={R}: routes {routes}")
    assert routes == routes_dup, f"the ROI list ran {routes}, the duplicate batch {routes_dup}"
    if dtype == "bf16" and not _routing_overrides():
        tower, cls = _expected_routes(R)
        assert routes == ([tower] * 3 if kind == "roienc" else [tower, tower, cls, AUX]), routes
    assert torch.equal(codes, want), f"codes differ: max |diff| {float((codes - want).abs().max())}"
    if wn is not None:
        assert torch.equal(wn, eng.codegen_weight_norm(len(seg_len)))
    for s in _stages(kind):
        w = eng.export_support(*s)
        assert got[s].shape == w.shape and got[s].shape[0] == (len(seg_len) if s[0] == "cls_tokens" else R), (s, got[s].shape)
        assert torch.equal(got[s], w), f"stage {s} differs from the duplicate batch"
    if ctx is not None:  # the context is per image: B rows; the duplicate batch has one per ROI
        assert tuple(ctx.shape) == (B, 256, 7, 7)
        assert torch.equal(ctx[torch.tensor(roi_image, device=ctx.device)], eng.export_support("context"))


# ------------------------------------------------------------------------------------------------ 2. ragged segments
def _ragged(kind, dtype, B, seg_len):
    R = sum(seg_len)
    feats = _pyramid(B, H, W, seed=40 + B)
    g = torch.Generator().manual_seed(R)
    roi_image = torch.randint(0, B, (R,), generator=g).tolist()
    boxes = _box_sets(R, H, W, seed=200 + R)[0]
    eng = _engine(kind, dtype=dtype)
    eng.import_pyramid(feats, (H, W))
    codes = eng.codegen_rois(boxes, roi_image, seg_len).clone()
    return eng, feats, roi_image, boxes, codes


def _check_ragged_codegen(kind, dtype, B, seg_len):
    R = sum(seg_len)
    eng, feats, roi_image, boxes, codes = _ragged(kind, dtype, B, seg_len)
    weighted = kind == "weighted"
    wn_got = eng.codegen_weight_norm(len(seg_len)).clone() if weighted else None
    taps = {s: eng.export_support(*s).clone() for s in (("roi", 0), ("conv_out", 0), ("conv_out", 1))}
    eng.import_pyramid(_dup(feats, roi_image), (H, W))
    eng.codegen_classes(boxes, 1)
    for s, t in taps.items():
        assert t.shape[0] == R and torch.equal(t, eng.export_support(*s)), f"per-ROI tap {s} differs from the duplicate batch"
    conv, aux = taps[("conv_out", 0)].cpu(), taps[("conv_out", 1)].cpu()
    assert aux.shape[1] == (3 if weighted else 1)
    r0 = 0
    for j, n in enumerate(seg_len):
        sl = slice(r0, r0 + n)
        want, wn, tol = codegen_tail_f64(conv[sl], aux[sl, 0:1], n, aux[sl, 1:2] if weighted else None, aux[sl, 2:3] if weighted else None,
                                         bias_l2_norm=weighted)
        assert_tail(codes[j:j + 1].cpu(), want, tol, f"{dtype} {kind} segment {j} ({n} shots) codegen tail")
        if weighted:
            err = abs(float(wn_got[j]) - float(wn[0]))
            print(f"segment {j}: cls_weight_norm {float(wn_got[j]):.6f} vs {float(wn[0]):.6f}")
            assert err <= 1e-5 * max(1.0, abs(float(wn[0]))), f"segment {j} cls_weight_norm: {err}"
        r0 += n


@pytest.mark.parametrize("kind", ["codegen", "weighted"])
def test_ragged_segments(kind):
    """R = 50 (no multiple of 16), segment lengths 1 ... 17 on 8 images."""
    _check_ragged_codegen(kind, "bf16", 8, [1, 2, 5, 9, 16, 17])


@pytest.mark.parametrize("kind", ["codegen", "weighted"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_segment_longer_than_64_shots(dtype, kind):
    """65 + 3 shots on 4 images: past the 64-shot cap of sylph_codegen_classes (strided softmax, weights beyond one wave); the weighted
    generator also checks cls_weight_norm of both segments against the scale head of codegen_tail_f64."""
    _check_ragged_codegen(kind, dtype, 4, [65, 3])


@pytest.mark.parametrize("seg_len,B", [([1, 2, 5, 9, 16, 17], 8), ([65, 3], 4)])
def test_ragged_segments_roi_encoder(seg_len, B):
    from oracle import bf16 as OB16
    R = sum(seg_len)
    eng, feats, roi_image, boxes, codes = _ragged("roienc", "bf16", B, seg_len)
    tok = eng.export_support("tokens", 2).cpu()
    cls = eng.export_support("cls_tokens").cpu()
    taps = {s: eng.export_support(*s).clone() for s in (("roi", 0), ("mscam", 0), ("tokens", 2))}
    assert tuple(tok.shape) == (R, 256) and tuple(cls.shape) == (len(seg_len), 256)
    want = torch.stack([tok[r0:r0 + n].double().mean(dim=0) for r0, n in zip([sum(seg_len[:j]) for j in range(len(seg_len))], seg_len)])
    assert_f32(cls, want, "class tokens of the ragged segments")
    sd64 = {k: v.double() for k, v in _state_dict("roienc").items()}
    assert_f32(codes.cpu(), OB16.roienc_heads(cls.double(), sd64), "code heads of the ragged segments")
    eng.import_pyramid(_dup(feats, roi_image), (H, W))
    eng.codegen_classes(boxes, 1)
    for s, t in taps.items():
        assert torch.equal(t, eng.export_support(*s)), f"per-ROI tap {s} differs from the duplicate batch"


# ------------------------------------------------------------------------------------------------ 3. one reference call per segment
@pytest.mark.parametrize("kind", ["codegen", "weighted", "roienc"])
def test_each_segment_is_one_reference_call(kind):
    B, seg_len = 4, [1, 3, 2, 4]
    R = sum(seg_len)
    feats = _pyramid(B, H, W, seed=7)
    roi_image = [3, 0, 0, 2, 1, 3, 2, 2, 0, 1]
    boxes = _box_sets(R, H, W, seed=300)[0]
    sd = _state_dict(kind)
    eng = _engine(kind, dtype="f32", taps=False)
    eng.import_pyramid(feats, (H, W))
    codes = eng.codegen_rois(boxes, roi_image, seg_len).clone().cpu()
    w = kind == "weighted"
    kw = {} if kind == "roienc" else dict(has_weight_layer=w, has_scale_layer=w, bias_l2_norm=w)
    oracle = segment_codes(kind, feats, boxes, roi_image, seg_len, sd, **kw)
    r0 = 0
    for j, n in enumerate(seg_len):
        eng.import_pyramid(_dup(feats, roi_image[r0:r0 + n]), (H, W))
        one = eng.codegen(boxes[r0:r0 + n]).cpu()
        assert_f32(codes[j], one, f"{kind} segment {j} vs a lone codegen call", rel=F32_REL)
        torch.testing.assert_close(codes[j], oracle[j], atol=1e-3, rtol=1e-3, msg=lambda m: f"{kind} segment {j} vs the fp32 oracle: {m}")
        r0 += n


# ------------------------------------------------------------------------------------------------ 4. ROIAlign edges
def _edge_rois():
    kinds = _box_kinds(H, W)
    level_boxes, outside = kinds[:5], kinds[9]
    assert [level_of_box(b.tolist()) for b in level_boxes] == [3, 4, 5, 6, 7]
    assert level_of_box(outside.tolist()) == 3 and float(outside[0]) > W + 200
    same = kinds[5]  # straddles the left border
    boxes = torch.cat([level_boxes, outside[None], same[None], same[None], kinds[11:13]])
    roi_image = [2, 0, 3, 3, 1, 2, 0, 3, 1, 1]
    return boxes, roi_image, 5, (6, 7)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_roi_align_rois_edges(dtype):
    B = 4
    feats = _pyramid(B, H, W, seed=11)
    boxes, roi_image, i_out, (s0, s1) = _edge_rois()
    eng = _engine("codegen", dtype=dtype, taps=False)
    eng.import_pyramid(feats, (H, W))
    got = eng.roi_align_rois(boxes, roi_image).clone()
    assert tuple(got.shape) == (len(roi_image), 256, 7, 7)
    assert float(got[i_out].abs().max()) == 0.0, "a box wholly outside its level must give exact zeros"
    assert roi_image[s0] != roi_image[s1] and not torch.equal(got[s0], got[s1]), "the same box on two images reads two images"
    one = eng.roi_align_rois(boxes[2:3], roi_image[2:3])  # R = 1
    assert torch.equal(one[0], got[2])
    dup = _dup(feats, roi_image)
    if dtype == "bf16":
        want = bf16_rne(torch.from_numpy(roi_pool_separable_f64([p.numpy() for p in dup], boxes.numpy(), f32_coords=True)))
        assert_ulps(got.cpu(), want, "ROIAlign over the ROI list")
    else:
        eng.import_pyramid(dup, (H, W))
        assert torch.equal(got, eng.roi_align(boxes)), "fp32: not the rows of sylph_roi_align on the duplicate batch"


# ------------------------------------------------------------------------------------------------ 5. call sequences
def _full_engine():
    from sylph_amd import synthetic as Wt
    from sylph_amd.engine import Engine
    eng = Engine(_cfg(), dtype="bf16")
    eng.load_state_dict(Wt.synthetic_state_dict(0, depth=50))
    return eng


def test_call_sequences_on_one_batch():
    from sylph_amd import synthetic as Wt
    B = 4
    feats = _pyramid(B, H, W, seed=21)
    g = torch.Generator().manual_seed(5)
    lists = {}
    for R, seg_len in ((10, [3, 7]), (50, [1, 2, 5, 9, 16, 17])):
        lists[R] = (_box_sets(R, H, W, seed=400 + R)[0], torch.randint(0, B, (R,), generator=g).tolist(), seg_len)
    one_box = _box_sets(B, H, W, seed=77)[0]
    qc = Wt.synthetic_codes(5, seed=77, scale=2.0)
    steps = {"rois10": lambda e: e.codegen_rois(*lists[10]).clone(), "rois50": lambda e: e.codegen_rois(*lists[50]).clone(),
             "codegen": lambda e: e.codegen(one_box).clone(), "classes": lambda e: e.codegen_classes(one_box, 2).clone()}

    def detect(e):
        e.head(qc["cls_conv"], qc["cls_bias"])
        return e.decode()

    alone = {}
    for name, fn in list(steps.items()) + [("detect", detect)]:
        e = _full_engine()
        e.import_pyramid(feats, (H, W))
        alone[name] = fn(e)
    eng = _full_engine()
    eng.import_pyramid(feats, (H, W))
    for name in ("rois10", "rois50", "codegen", "rois10", "classes", "rois50"):
        assert torch.equal(steps[name](eng), alone[name]), f"{name} in a sequence differs from the call alone"
    dets = detect(eng)
    assert sum(int(d["scores"].numel()) for d in dets) > 0
    for d, w in zip(dets, alone["detect"]):
        for k in w:
            assert torch.equal(d[k], w[k]), f"decode after ROI-list calls: {k} differs"
    assert torch.equal(steps["rois50"](eng), alone["rois50"]), "a ROI-list call after head + decode differs from the call alone"
    # tables: a repeated identical list uploads nothing (counted by the library, not timed); another list of the same R does
    n0 = eng.roi_table_uploads()
    for _ in range(3):
        assert torch.equal(steps["rois50"](eng), alone["rois50"])
    assert eng.roi_table_uploads() == n0
    bx, ri, sl = lists[50]
    eng.codegen_rois(bx, ri[::-1], sl)
    assert eng.roi_table_uploads() == n0 + 1
    eng.codegen_rois(bx, ri[::-1], sl[::-1])
    assert eng.roi_table_uploads() == n0 + 2
    assert torch.equal(steps["rois50"](eng), alone["rois50"]) and eng.roi_table_uploads() == n0 + 3
    # R = B: a scattered ROI list of 4 rows shares its pass and its tables with codegen and codegen_classes(., 2); a stale image or
    # segment table of the call before would show in the next one
    lists[4] = (_box_sets(4, H, W, seed=404)[0], [2, 0, 3, 0], [1, 3])
    steps["rois4"] = lambda e: e.codegen_rois(*lists[4]).clone()
    e = _full_engine()
    e.import_pyramid(feats, (H, W))
    alone["rois4"] = steps["rois4"](e)
    assert not torch.equal(alone["rois4"][:1], alone["codegen"].reshape(1, -1))
    for name in ("rois4", "codegen", "rois4", "classes", "rois4", "classes", "codegen", "rois4"):
        assert torch.equal(steps[name](eng), alone[name]), f"{name} in the R = B sequence differs from the call alone"


# ------------------------------------------------------------------------------------------------ 5b. the parent's bits
def test_class_form_equals_the_parent(golden_dir):
    """codegen, codegen_classes and roi_align run as ROI lists (roi_image[r] = r, equal segments) and give bit for bit what their own
    kernels gave on an MI355X with the library of the commit before (g12_parent_support.npz,
    tests/golden/gen_parent_support_golden.py): codes, cls_weight_norm, the ROIEncoder's class tokens, the pooled edge boxes."""
    from support_parent_ref import outputs_support
    want = np.load(os.path.join(golden_dir, "g12_parent_support.npz"))
    got = outputs_support()
    assert sorted(got) == sorted(want.files)
    for k in want.files:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), f"{k} differs from the parent's"
    for k in want.files:
        if k.endswith("_codes"):
            assert float(np.abs(want[k]).max()) > 0, f"{k}: the stored codes are all zero"


# ------------------------------------------------------------------------------------------------ 6. errors
def test_invalid_roi_lists_raise_and_change_nothing():
    from sylph_amd._lib import lib
    B = 4
    feats = _pyramid(B, H, W, seed=31)
    boxes = _box_sets(6, H, W, seed=500)[0]
    roi_image, seg_len = [0, 3, 3, 1, 2, 0], [2, 4]
    eng = _engine("weighted", taps=False)
    with pytest.raises(ValueError, match="no current batch"):
        eng.codegen_rois(boxes, roi_image, seg_len)
    eng.import_pyramid(feats, (H, W))
    before = eng.codegen_rois(boxes, roi_image, seg_len).clone()
    wn = eng.codegen_weight_norm(2).clone()
    n0 = eng.roi_table_uploads()
    bad = [((boxes, [0, 3, 4, 1, 2, 0], seg_len), r"roi_image\[2\] = 4"), ((boxes, [0, 3, 3, 1, 2, -1], seg_len), r"roi_image\[5\] = -1"),
           ((boxes, roi_image, [2, 0, 4]), r"seg_len\[1\] = 0"), ((boxes, roi_image, [6, -1, 1]), r"seg_len\[1\] = -1"),
           ((boxes, roi_image, [2, 3]), "sum to 5"), ((boxes, roi_image, [2, 5]), "sum to 7"), ((boxes[:0], [], []), "R < 1"),
           ((boxes, roi_image, []), "n_seg < 1"), ((None, roi_image, seg_len), "must be given"), ((boxes, None, seg_len), "must be given"),
           ((boxes, roi_image, None), "must be given"), ((boxes[:5], roi_image, seg_len), "20 values for 6 ROIs")]
    for args, msg in bad:
        with pytest.raises(ValueError, match=msg):
            eng.codegen_rois(*args)
    for args in ((boxes, [0, 3, 4, 1, 2, 0]), (boxes[:0], []), (None, roi_image), (boxes, None)):
        with pytest.raises(ValueError):
            eng.roi_align_rois(*args)
    # the C ABI makes the same checks for callers that do not come through the engine: non-zero return, the index in the message
    L = lib()
    bx = boxes.cuda().contiguous()
    out = torch.empty(2, 257, device="cuda")
    I = lambda v: (ctypes.c_int * max(len(v), 1))(*v)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    for R, bp, ri, ns, sl, op, msg in ((6, P(bx), I([0, 3, 4, 1, 2, 0]), 2, I(seg_len), P(out), "roi_image[2] = 4"),
                                       (6, P(bx), I(roi_image), 3, I([2, 0, 4]), P(out), "seg_len[1] = 0"),
                                       (6, P(bx), I(roi_image), 2, I([2, 3]), P(out), "sum to 5"),
                                       (0, P(bx), I(roi_image), 2, I(seg_len), P(out), "R = 0"),
                                       (6, P(bx), I(roi_image), 0, I(seg_len), P(out), "n_seg = 0"),
                                       (6, None, I(roi_image), 2, I(seg_len), P(out), "NULL"), (6, P(bx), None, 2, I(seg_len), P(out), "NULL"),
                                       (6, P(bx), I(roi_image), 2, None, P(out), "NULL"), (6, P(bx), I(roi_image), 2, I(seg_len), None, "NULL")):
        assert L.sylph_codegen_rois(eng._ctx, R, bp, ri, ns, sl, op) != 0
        assert msg in L.sylph_last_error().decode(), (msg, L.sylph_last_error().decode())
    assert L.sylph_roi_align_rois(eng._ctx, 6, P(bx), I([0, 9, 0, 0, 0, 0]), P(out)) != 0 and "roi_image[1] = 9" in L.sylph_last_error().decode()
    # nothing changed: the state of the last valid call is still there, and the same call gives the same codes without a new upload
    assert torch.equal(eng.codegen_weight_norm(2), wn)
    assert torch.equal(eng.codegen_rois(boxes, roi_image, seg_len), before)
    assert eng.roi_table_uploads() == n0


# ------------------------------------------------------------------------------------------------ 7. model level
def _annotated_records(seed=3):
    """Five 128 x 160 records with 2, 3, 1, 2, 1 boxes of classes 4, 1, 6 (first appearance in that order)."""
    from sylph_amd import synthetic as Wt
    from sylph_amd.structures import Boxes, Instances
    spec = [[4, 1], [1, 4, 6], [6], [4, 4], [1]]
    recs = []
    for i, cls in enumerate(spec):
        inst = Instances((128, 160))
        inst.gt_boxes = Boxes(torch.tensor([[6.0 + 9 * i + 5 * k, 4.0 + 7 * k, 70.0 + 20 * k + 3 * i, 60.0 + 15 * k + i] for k in range(len(cls))]))
        inst.gt_classes = torch.tensor(cls)
        recs.append({"image": Wt.synthetic_images(1, 128, 160, seed=seed * 10 + i)[0], "instances": inst, "height": 128, "width": 160})
    return recs


def test_model_class_codes_from_roi_segments():
    from sylph_amd import synthetic as Wt
    from sylph_amd.evaluation import inference_on_annotated_images, plan_roi_segments
    from sylph_amd.runner import MetaFCOSRunner, create_cfg
    from sylph_amd.structures import Boxes, Instances
    runner = MetaFCOSRunner()
    cfg = create_cfg(runner.get_default_cfg(), "sylph://COCO-Detection/Meta-FCOS/Meta-FCOS-finetune.yaml")
    m = runner.build_model(cfg, dtype="f32")
    m.load_state_dict(Wt.synthetic_state_dict(0, depth=50))
    m.eval()
    m.engine.profile_enable(True)
    recs = _annotated_records()[:3]
    box = lambda i, k: recs[i]["instances"].gt_boxes.tensor[k]
    pairs = [[(0, 0), (1, 1)], [(1, 0), (2, 0)], [(0, 1), (1, 2)]]  # segments mix images; image 1 serves all three
    segments = [{"image_index": torch.tensor([i for i, _ in p]), "boxes": torch.stack([box(i, k) for i, k in p])} for p in pairs]
    with pytest.raises(ValueError, match="segment 1 is empty"):
        m.forward_class_codes_rois(recs, [segments[0], {"image_index": torch.zeros(0, dtype=torch.long), "boxes": torch.zeros(0, 4)}])
    np.random.seed(1234)  # select_a_mask's generator (forward_class_code draws from it for a record with several boxes)
    got = [{k: v.clone() for k, v in c.items()} for c in m.forward_class_codes_rois(recs, segments)]
    drawn = np.random.randint(1 << 30)
    np.random.seed(1234)
    assert drawn == np.random.randint(1 << 30), "forward_class_codes_rois drew from the global generator"
    routes_rois = m.engine.conv_routes()
    assert len(got) == 3
    for j, p in enumerate(pairs):
        sup = []
        for i, k in p:  # the image once per instance, each copy with its single box: forward_class_code draws nothing
            inst = Instances((128, 160))
            inst.gt_boxes = Boxes(box(i, k).reshape(1, 4))
            inst.gt_classes = torch.tensor([0])
            sup.append({"image": recs[i]["image"], "instances": inst, "height": 128, "width": 160})
        want = m([{"support_set": sup, "support_set_target": torch.tensor(j), "class_name": str(j)}], run_type="meta_learn_test_support")
        routes_one = m.engine.conv_routes()
        assert tuple(got[j]["cls_conv"].shape) == tuple(want["cls_conv"].shape) == (1, 256, 1, 1)
        assert tuple(got[j]["cls_bias"].shape) == tuple(want["cls_bias"].shape) == (1, 1, 1, 1)
        for k in ("cls_conv", "cls_bias"):
            if not torch.equal(got[j][k], want[k]):
                diff = [(a, b) for a, b in zip(routes_rois, routes_one) if a != b] if j == 0 else "(routes of the first call)"
                err, scale = float((got[j][k] - want[k]).abs().max()), max(1.0, float(want[k].abs().max()))
                print(f"segment {j} {k}: max |diff| {err:.3e}; conv routes that differ (ROI list, one class per call): {diff}")
                assert j > 0 or diff, f"segment {j} {k} differs by {err} although both sides took the same conv routes"
                assert err <= F32_REL * scale, f"segment {j} {k}: {err} > {F32_REL} * {scale}; conv routes that differ: {diff}"

    # the evaluation loop: two loader items, every instance a shot of its class, chunks of at most 2
    all_recs = _annotated_records()
    items = [all_recs[:3], all_recs[3:]]
    names = {4: "four", 1: "one", 6: "six"}
    sums, counts = {}, {}
    for it in items:
        boxes, roi_image, seg_len, seg_class = plan_roi_segments(it, chunk=2)
        segs, r0 = [], 0
        for n in seg_len:
            segs.append({"image_index": torch.tensor(roi_image[r0:r0 + n]), "boxes": boxes[r0:r0 + n]})
            r0 += n
        for c, n, cid in zip(m.forward_class_codes_rois(it, segs), seg_len, seg_class):
            row = torch.cat([c["cls_conv"].reshape(-1), c["cls_bias"].reshape(-1)]).double().cpu() * n
            sums[cid] = sums.get(cid, 0) + row
            counts[cid] = counts.get(cid, 0) + n
    assert counts == {4: 4, 1: 3, 6: 2}
    out = inference_on_annotated_images(m, items, chunk=2, class_names=names)
    assert [r["support_set_target"] for r in out] == [4, 1, 6] and [r["class_name"] for r in out] == ["four", "one", "six"]
    for r in out:
        cc = r["class_code"]
        assert set(r) == {"support_set_target", "class_name", "class_code"} and set(cc) == {"cls_conv", "cls_bias", "acc_weight"}
        assert tuple(cc["cls_conv"].shape) == (1, 256, 1, 1) and tuple(cc["cls_bias"].shape) == (1, 1, 1, 1) and not cc["cls_conv"].is_cuda
        assert cc["acc_weight"] == 1.0
        want = sums[r["support_set_target"]] / counts[r["support_set_target"]]
        row = torch.cat([cc["cls_conv"].reshape(-1), cc["cls_bias"].reshape(-1)])
        # (n1 c1 + n2 c2) / n in fp32: the products by 1 or 2 are exact, one rounding for the sum, one for the division: 2^-23 relative
        assert_f32(row, want, f"class {r['class_name']}: count-weighted mean of its chunk codes", rel=1e-6)
