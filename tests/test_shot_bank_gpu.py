"""Shot bank on the GPU (sylph_codegen_shots / sylph_shot_combine): per-shot rows kept, class codes of any draw from a gather.

What is under test is an identity, not an approximation: combine_shots over the rows of codegen_shots repeats the operations of
codegen_rois' last kernel in their order (csrc/shot_bank.hip, built without FMA contraction like csrc/codegen.hip), so every comparison
with codegen_rois here is torch.equal.  The rows themselves and the combination of rows that no single batch holds are compared bit for
bit with the float32 restatement tests/shot_bank_ref.py where the arithmetic is IEEE-specified (sums, products, divisions, square
roots); the softmax's expf is another libm than numpy's, so the WEIGHT_LAYER combination is pinned by the codegen_rois identities
(tests 1 - 3) and not by the restatement.
Pyramids go in through Engine.import_pyramid at 64 x 96 and 96 x 64, as in tests/test_support_rois_gpu.py."""
import ctypes

import numpy as np
import pytest
import torch

import shot_bank_ref as SB
from test_support_bf16_pinned_gpu import _box_sets, _cfg, _pyramid

pytestmark = pytest.mark.gpu

H, W = 64, 96
KINDS = ["plain", "weighted", "l2", "k3", "roienc"]
ROI_IMAGE = [2, 0, 2, 2, 0, 2, 0]  # B = 3: image 0 carries 3 ROIs, image 1 none, image 2 four; scattered
SEG_LEN = [3, 1, 3]


def _engine(kind, dtype="bf16", full=False):
    """plain | weighted (WEIGHT_LAYER + SCALE_LAYER) | l2 (BIAS_L2_NORM) | k3 (CLS_LAYER kernel size 3) | roienc; full: the whole
    synthetic network's weights (the query head too), else the generator's alone"""
    from sylph_amd import synthetic as Wt
    from sylph_amd.engine import Engine
    cfg = _cfg(roi_encoder=kind == "roienc")
    cg = cfg.MODEL.META_LEARN.CODE_GENERATOR
    if kind == "weighted":
        cg.WEIGHT_LAYER, cg.SCALE_LAYER = ["", "", 1], ["", "", 1]
    if kind == "l2":
        cg.BIAS_L2_NORM = True
    if kind == "k3":
        cg.CLS_LAYER = ["", "", 3]
    eng = Engine(cfg, dtype=dtype)
    sd = Wt.synthetic_state_dict(0, depth=50) if full else {}
    sd.update(Wt.roi_encoder_state_dict(seed=4) if kind == "roienc" else Wt.codegen_state_dict(seed=2, weight_scale_layers=kind == "weighted"))
    eng.load_state_dict(sd)
    return eng


def _batch(eng, B=3, hw=(H, W), seed=3):
    eng.import_pyramid(_pyramid(B, hw[0], hw[1], seed=seed), hw)


def _rois(eng, boxes, roi_image, seg_len):
    codes = eng.codegen_rois(boxes, roi_image, seg_len).clone()
    wn = eng.codegen_weight_norm(len(seg_len)).clone() if int(eng.sc.cg_has_scale) and not eng.is_roi_encoder else None
    return codes, wn


def _same(got, want, what):
    (codes, wn), (wcodes, wwn) = got, want
    assert codes.shape == wcodes.shape
    assert torch.equal(codes, wcodes), f"{what}: codes differ, max |diff| {float((codes - wcodes).abs().max())}"
    assert (wn is None) == (wwn is None)
    if wn is not None:
        assert torch.equal(wn, wwn), f"{what}: cls_weight_norm differs"


# ------------------------------------------------------------------------------------------------ 1. identity
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", ["f32", "f32s", "bf16"])
def test_bank_of_a_list_gives_the_codes_of_the_list(dtype, kind):
    eng = _engine(kind, dtype)
    _batch(eng)
    boxes = _box_sets(7, H, W, seed=107)[0]
    want = _rois(eng, boxes, ROI_IMAGE, SEG_LEN)
    n0 = eng.roi_table_uploads()
    rows = eng.codegen_shots(boxes, ROI_IMAGE)
    assert tuple(rows.shape) == (7, eng.shot_row_floats) and eng.shot_row_floats == (260 if kind != "k3" else 2308)
    assert eng.roi_table_uploads() == n0, "codegen_shots on the list of the call before uploaded tables"
    assert float(rows[:, -1].abs().max()) == 0.0, "the pad float"
    _same(eng.combine_shots(rows, torch.arange(7), SEG_LEN), want, f"{dtype} {kind}")
    assert float(want[0].abs().max()) > 0
    _same(_rois(eng, boxes, ROI_IMAGE, SEG_LEN), want, "codegen_rois after codegen_shots")
    assert eng.roi_table_uploads() == n0, "codegen_rois with the same list after codegen_shots uploaded tables"


# ------------------------------------------------------------------------------------------------ 2. draws
@pytest.mark.parametrize("kind", KINDS)
def test_permuted_and_repeated_draw(kind):
    eng = _engine(kind)
    _batch(eng)
    boxes = _box_sets(7, H, W, seed=107)[0]
    rows = eng.codegen_shots(boxes, ROI_IMAGE).clone()
    idx, seg_len = [6, 0, 0, 3, 5, 1], [2, 4]
    got = eng.combine_shots(rows, idx, seg_len)
    want = _rois(eng, boxes[idx], [ROI_IMAGE[i] for i in idx], seg_len)
    _same(got, want, f"{kind} draw {idx}")
    other = eng.combine_shots(rows, [2, 4, 0, 3, 5, 1], seg_len)[0]  # another first segment: the second does not notice
    assert torch.equal(other[1], got[0][1]) and not torch.equal(other[0], got[0][0])


# ------------------------------------------------------------------------------------------------ 3. long segment
@pytest.mark.parametrize("kind", ["weighted", "roienc"])
def test_segment_of_130_repeated_shots(kind):
    """130 shots in one segment: every lane of the softmax owns two or three shots and the weights fill more than 64 LDS slots.
    The yardstick, codegen_rois with R = 131, runs its convolutions on other tiles than a 7-ROI call (igemm 64x128 instead of 64x64 in
    bf16: the routes follow the row count), and a conv output differs between routes in its last bits (measured: rows up to 1.7e-6
    apart, codes 4.8e-7).  The seven bank rows are therefore made by a call of the yardstick's size -- the seven ROIs first, then
    repeats -- so that both sides start from the same per-shot values; what is compared is then the combination alone."""
    eng = _engine(kind)
    _batch(eng)
    boxes = _box_sets(7, H, W, seed=107)[0]
    g = torch.Generator().manual_seed(130)
    idx = torch.randint(0, 7, (130,), generator=g).tolist() + [4]
    assert set(idx[:130]) == set(range(7))
    fill = list(range(7)) + [i % 7 for i in range(124)]
    rows = eng.codegen_shots(boxes[fill], [ROI_IMAGE[i] for i in fill])[:7].clone()  # (the pass codegen_rois runs below: the plan's, for R = 131)
    got = eng.combine_shots(rows, idx, [130, 1])
    want = _rois(eng, boxes[idx], [ROI_IMAGE[i] for i in idx], [130, 1])  # R = 131 on the same batch
    _same(got, want, f"{kind} 130 + 1")


# ------------------------------------------------------------------------------------------------ 4. rows and cross-call banks
def _heads(kind):
    return dict(ib=0, iw=1 if kind == "weighted" else -1, is_=2 if kind == "weighted" else -1, k=3 if kind == "k3" else 1, bias_l2_norm=kind == "l2")


@pytest.mark.parametrize("kind", ["plain", "weighted", "l2", "k3"])
def test_rows_are_the_restated_pool_of_the_conv_taps(kind):
    eng = _engine(kind)
    _batch(eng)
    boxes = _box_sets(7, H, W, seed=107)[0]
    rows = eng.codegen_shots(boxes, ROI_IMAGE).clone()
    conv, aux = eng.export_support("conv_out", 0).cpu().numpy(), eng.export_support("conv_out", 1).cpu().numpy()
    assert conv.shape == (7, 256, 7, 7) and aux.shape == (7, 3 if kind == "weighted" else 1, 7, 7)
    want = SB.pool_rows(conv, aux, **_heads(kind))
    got = rows.cpu().numpy()
    n = want.shape[1] - 4
    for name, sl in (("conv map", slice(0, n)), ("bias term", slice(n, n + 1)), ("logit", slice(n + 1, n + 2)), ("scale term", slice(n + 2, n + 3)),
                     ("pad", slice(n + 3, n + 4))):
        assert np.array_equal(got[:, sl], want[:, sl]), f"{kind} {name}: max |diff| {np.abs(got[:, sl] - want[:, sl]).max()}"
    assert np.abs(got[:, :n]).max() > 0 and np.abs(got[:, n]).max() > 0
    if kind == "weighted":
        assert np.abs(got[:, n + 1]).max() > 0 and np.abs(got[:, n + 2]).max() > 0


@pytest.mark.parametrize("kind", ["plain", "l2", "k3", "roienc"])
def test_bank_from_two_batches_of_two_sizes(kind):
    """Rows of two calls on two batches of different image sizes, concatenated; segments mix rows of both.  No single batch holds these
    shots, so the yardstick is the restatement's combine of the downloaded rows (the ROIEncoder: the codes of segments that stay
    inside one part equal that part's own codegen_rois).  The same again while a query record is the current batch."""
    eng = _engine(kind, full=True)
    _batch(eng, B=3, hw=(H, W), seed=3)
    boxes_a = _box_sets(7, H, W, seed=107)[0]
    rows_a = eng.codegen_shots(boxes_a, ROI_IMAGE).clone()
    codes_a = _rois(eng, boxes_a, ROI_IMAGE, SEG_LEN)
    _batch(eng, B=2, hw=(W, H), seed=5)
    boxes_b = _box_sets(5, W, H, seed=205)[0]
    roi_b = [1, 0, 0, 1, 1]
    rows_b = eng.codegen_shots(boxes_b, roi_b).clone()
    bank = torch.cat([rows_a, rows_b]).contiguous()
    idx, seg_len = [8, 1, 11, 0, 7, 7, 3, 2, 10, 9, 4, 5, 6], [4, 1, 5, 3]
    assert any(i < 7 for i in idx[:4]) and any(i >= 7 for i in idx[:4])

    def check(what):
        got = eng.combine_shots(bank, idx, seg_len)
        if kind == "roienc":
            assert got[1] is None
            _same(eng.combine_shots(bank, list(range(7)), SEG_LEN), codes_a, f"{what}: part a inside the bank")
            assert float(got[0].abs().max()) > 0
        else:
            want, _ = SB.combine_rows(bank.cpu().numpy(), idx, seg_len, k=3 if kind == "k3" else 1)
            assert np.array_equal(got[0].cpu().numpy(), want), f"{what}: max |diff| {np.abs(got[0].cpu().numpy() - want).max()}"
        return got[0].clone()

    fresh = check(f"{kind} mixed bank")
    eng.towers()
    rec = eng.store_record()
    eng.load_record(rec)
    assert torch.equal(check(f"{kind} mixed bank on a loaded record"), fresh)
    with pytest.raises(RuntimeError, match="sylph_codegen_shots.*query record"):
        eng.codegen_shots(boxes_b, roi_b)
    rec.close()


# ------------------------------------------------------------------------------------------------ 5. errors
def test_invalid_draws_raise_and_launch_nothing():
    from sylph_amd._lib import lib
    eng = _engine("weighted")
    boxes = _box_sets(7, H, W, seed=107)[0]
    with pytest.raises(ValueError, match="no current batch"):
        eng.codegen_shots(boxes, ROI_IMAGE)
    _batch(eng)
    with pytest.raises(ValueError, match=r"roi_image\[1\] = 3"):
        eng.codegen_shots(boxes, [2, 3, 2, 2, 0, 2, 0])
    rows = eng.codegen_shots(boxes, ROI_IMAGE).clone()
    good = eng.combine_shots(rows, [0, 1, 2], [2, 1])
    bad = [((rows, [0, 7, 2], [2, 1]), r"idx\[1\] = 7 is outside the bank of 7 rows"), ((rows, [0, -1, 2], [2, 1]), r"idx\[1\] = -1"),
           ((rows, [0, 1, 2], [3, 0]), r"seg_len\[1\] = 0"), ((rows, [0, 1, 2], [2, 2]), "sum to 4, not to M = 3"),
           ((rows, [0, 1, 2], []), "n_seg < 1"), ((rows[:, :257].contiguous(), [0, 1, 2], [2, 1]), "bank rows of 257 floats.*260 floats wide"),
           ((None, [0], [1]), "must be given")]
    for args, msg in bad:
        with pytest.raises(ValueError, match=msg):
            eng.combine_shots(*args)
    # the C ABI makes the same checks on the host, before anything is copied or launched: non-zero return, the position in the message,
    # and an output buffer that nobody wrote
    L = lib()
    out = torch.full((2, 257), 7.0, device="cuda")
    wn = torch.full((2,), 7.0, device="cuda")
    I = lambda v: (ctypes.c_int * max(len(v), 1))(*v)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    long_seg = [16385, 1]
    for n_rows, M, ix, ns, sl, msg in ((7, 3, I([0, 7, 2]), 2, I([2, 1]), "idx[1] = 7"), (7, 3, I([0, 1, 2]), 2, I([3, 0]), "seg_len[1] = 0"),
                                       (7, 3, I([0, 1, 2]), 2, I([2, 2]), "sum to 4"), (7, 3, I([0, 1, 2]), 0, I([3]), "n_seg = 0"),
                                       (7, 16386, I([0] * 16386), 2, I(long_seg), "seg_len[0] = 16385"), (0, 3, I([0, 1, 2]), 1, I([3]), "n_rows = 0"),
                                       (7, 3, None, 1, I([3]), "NULL"), (7, 3, I([0, 1, 2]), 1, None, "NULL")):
        assert L.sylph_shot_combine(eng._ctx, P(rows), n_rows, M, ix, ns, sl, P(out), P(wn)) != 0
        assert msg in L.sylph_last_error().decode(), (msg, L.sylph_last_error().decode())
    assert L.sylph_shot_combine(eng._ctx, None, 7, 3, I([0, 1, 2]), 1, I([3]), P(out), P(wn)) != 0 and "NULL" in L.sylph_last_error().decode()
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 and float(out.max()) == 7.0 and float(wn.min()) == 7.0, "a refused call wrote its outputs"
    _same(eng.combine_shots(rows, [0, 1, 2], [2, 1]), good, "after the refused calls")
    # weight_norm_out may be NULL
    assert L.sylph_shot_combine(eng._ctx, P(rows), 7, 3, I([0, 1, 2]), 2, I([2, 1]), P(out), None) == 0
    assert torch.equal(out, good[0])


# ------------------------------------------------------------------------------------------------ 6. end to end
def _records():
    """Four 128 x 160 annotated records, classes 0, 1, 2 with 4, 2 and 2 instances"""
    from sylph_amd import synthetic as Wt
    from sylph_amd.structures import Boxes, Instances
    spec = [[0, 1], [1, 0, 2], [2], [0, 0]]
    recs = []
    for i, cls in enumerate(spec):
        inst = Instances((128, 160))
        inst.gt_boxes = Boxes(torch.tensor([[6.0 + 9 * i + 5 * k, 4.0 + 7 * k, 70.0 + 20 * k + 3 * i, 60.0 + 15 * k + i] for k in range(len(cls))]))
        inst.gt_classes = torch.tensor(cls)
        recs.append({"image": Wt.synthetic_images(1, 128, 160, seed=80 + i)[0], "instances": inst, "height": 128, "width": 160, "image_id": 100 + i})
    return recs


def test_bank_draws_detect_like_fresh_support_passes():
    from sylph_amd import synthetic as Wt
    from sylph_amd.evaluation import (build_shot_bank, class_codes_from_bank, format_class_codes_shared, inference_normalization,
                                      inference_on_annotated_images)
    from sylph_amd.runner import MetaFCOSRunner, create_cfg
    from sylph_amd.structures import Boxes, Instances
    runner = MetaFCOSRunner()
    cfg = create_cfg(runner.get_default_cfg(), "sylph://COCO-Detection/Meta-FCOS/Meta-FCOS-finetune.yaml")
    m = runner.build_model(cfg, dtype="f32")
    m.load_state_dict(Wt.synthetic_state_dict(0, depth=50))
    m.eval()
    m.engine.profile_enable(True)
    recs = _records()
    bank = build_shot_bank(m, [recs])
    routes_bank = m.engine.conv_routes()
    assert len(bank) == 8 and bank.classes() == [0, 1, 2] and bank.image_ids == [100, 100, 101, 101, 101, 102, 103, 103]
    assert bank.ann_ids == [0, 1, 0, 1, 2, 0, 0, 1] and bank.nbytes == 8 * 260 * 4
    query = [{"image": Wt.synthetic_images(1, 128, 160, seed=9)[0], "height": 128, "width": 160}]
    n_det = 0
    for shots, seed in ((1, 3), (2, 5)):  # at most two shots per class: the sum of two terms does not depend on their order
        idx, seg_len, class_ids = bank.draw(shots, seed)
        assert seg_len == [shots] * 3 and class_ids == [0, 1, 2]
        codes = format_class_codes_shared(class_codes_from_bank(m, bank, idx, seg_len, class_ids), device=m.device)
        got = m(query, class_code=codes, run_type="meta_learn_test_instance")[0]["instances"]
        # the fresh support pass over the same four images, annotated with the drawn instances alone
        keep = {(bank.image_ids[r], bank.ann_ids[r]) for r in idx}
        sub = []
        for rec in recs:
            sel = [a for a in range(len(rec["instances"].gt_classes)) if (rec["image_id"], a) in keep]
            inst = Instances((128, 160))
            inst.gt_boxes = Boxes(rec["instances"].gt_boxes.tensor[sel].reshape(-1, 4))
            inst.gt_classes = rec["instances"].gt_classes[sel]
            sub.append(dict(rec, instances=inst))
        fresh = inference_on_annotated_images(m, [sub])
        for r in fresh:
            assert r["class_code"].pop("acc_weight") == 1.0  # (the reduce's bookkeeping, a float: not a code field)
        fresh = inference_normalization(m, fresh)
        routes_fresh = m.engine.conv_routes()
        want_codes = format_class_codes_shared(fresh, device=m.device)
        why = f"draw ({shots}, {seed}); conv routes of the bank build {routes_bank}, of the fresh pass {routes_fresh}"
        for k in ("cls_conv", "cls_bias"):
            assert torch.equal(codes[k], want_codes[k]), f"{k} differs, max |diff| {float((codes[k] - want_codes[k]).abs().max())}; {why}"
        want = m(query, class_code=want_codes, run_type="meta_learn_test_instance")[0]["instances"]
        assert torch.equal(got.pred_boxes.tensor, want.pred_boxes.tensor), why
        assert torch.equal(got.scores, want.scores) and torch.equal(got.pred_classes, want.pred_classes), why
        n_det += len(want)
    assert n_det > 0, "no detections at all: the comparison is empty"
