"""Host side of the ROI-list support path: the segment planner, the gather-and-loop reference the GPU tests compare against, and the
C ABI declarations.  No GPU."""
import os
import re

import pytest
import torch

from support_rois_ref import gather_segment, segment_code_dicts, segment_codes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _record(boxes_classes, hw=(64, 96)):
    from sylph_amd.structures import Boxes, Instances
    inst = Instances(hw)
    inst.gt_boxes = Boxes(torch.tensor([b for b, _ in boxes_classes], dtype=torch.float32).reshape(-1, 4))
    inst.gt_classes = torch.tensor([c for _, c in boxes_classes], dtype=torch.int64)
    return {"image": torch.zeros(3, *hw), "instances": inst}


def _box(i):
    return [float(i), float(2 * i), float(i + 10), float(2 * i + 20)]


def _records():
    """image 0: classes 7, 3, 7, 5 (three classes, 7 twice); image 1: no boxes; image 2: class 3; image 3: classes 5, 7, 7;
    image 4: a record without "instances"; image 5: class 9.  Class 7 is spread over the non-adjacent images 0 and 3."""
    return [_record([(_box(0), 7), (_box(1), 3), (_box(2), 7), (_box(3), 5)]),
            _record([]),
            _record([(_box(4), 3)]),
            _record([(_box(5), 5), (_box(6), 7), (_box(7), 7)]),
            {"image": torch.zeros(3, 64, 96)},
            _record([(_box(8), 9)])]


# class -> its shots (image, box id) in image order, then box order; classes in order of first appearance
WANT = [(7, [(0, 0), (0, 2), (3, 6), (3, 7)]), (3, [(0, 1), (2, 4)]), (5, [(0, 3), (3, 5)]), (9, [(5, 8)])]


@pytest.mark.parametrize("chunk", [1, 2, 3, 100])
def test_plan_roi_segments(chunk):
    from sylph_amd.evaluation import plan_roi_segments
    boxes, roi_image, seg_len, seg_class = plan_roi_segments(_records(), chunk=chunk)
    want_img, want_box, want_len, want_cls = [], [], [], []
    for cid, shots in WANT:
        for k in range(0, len(shots), chunk):
            part = shots[k:k + chunk]
            want_img += [b for b, _ in part]
            want_box += [_box(i) for _, i in part]
            want_len.append(len(part))
            want_cls.append(cid)
    assert roi_image == want_img and seg_len == want_len and seg_class == want_cls
    assert sum(seg_len) == len(roi_image) == boxes.shape[0] == 9 and max(seg_len) <= chunk and min(seg_len) >= 1
    assert boxes.dtype == torch.float32 and torch.equal(boxes, torch.tensor(want_box))
    assert all(isinstance(v, int) for v in roi_image + seg_len + seg_class)
    again = plan_roi_segments(_records(), chunk=chunk)  # deterministic: nothing is drawn
    assert torch.equal(again[0], boxes) and again[1:] == (roi_image, seg_len, seg_class)


def test_plan_roi_segments_edges():
    from sylph_amd.evaluation import plan_roi_segments
    boxes, roi_image, seg_len, seg_class = plan_roi_segments([_record([]), {"image": torch.zeros(3, 8, 8)}])
    assert tuple(boxes.shape) == (0, 4) and roi_image == [] and seg_len == [] and seg_class == []
    with pytest.raises(ValueError):
        plan_roi_segments(_records(), chunk=0)
    # the default chunk is the base-class path's 10
    many = [_record([(_box(i), 1) for i in range(7)]), _record([(_box(i), 1) for i in range(16)])]
    _, roi_image, seg_len, seg_class = plan_roi_segments(many)
    assert seg_len == [10, 10, 3] and seg_class == [1, 1, 1] and roi_image == [0] * 7 + [1] * 16


# ------------------------------------------------------------------------------------------------ the gather-and-loop reference
def _toy(B=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    feats = [torch.randn(B, 256, 12, 16, generator=g), torch.randn(B, 256, 6, 8, generator=g)]  # strides 8, 16 of a 96 x 128 image
    # sqrt(area) < 224: level 3 (stride 8); >= 224: level 4.  Image 1 is used three times, image 2 never, the order is not monotonic
    boxes = torch.tensor([[8.0, 6.0, 70.0, 60.0], [0.0, 0.0, 128.0, 96.0], [-20.0, 10.0, 300.0, 280.0], [30.5, 20.25, 90.0, 81.0],
                          [5.0, 5.0, 250.0, 230.0]])
    roi_image = [1, 0, 1, 1, 0]
    return feats, boxes, roi_image, [2, 3]


def test_gather_segment_indexing():
    feats, _, roi_image, seg_len = _toy()
    got = gather_segment(feats, roi_image, 2, 3)
    for f, g in zip(feats, got):
        assert tuple(g.shape) == (3,) + tuple(f.shape[1:])
        for i, b in enumerate(roi_image[2:5]):
            assert torch.equal(g[i], f[b])


@pytest.mark.parametrize("kind", ["codegen", "weighted", "roienc"])
def test_reference_equals_oracle_on_duplicated_images(kind):
    """Per segment the restatement must be the oracle's one-class call on a batch that holds the segment's images explicitly, once per
    ROI -- built here with python indexing and torch.stack, not with index_select."""
    from oracle import codegen as CG, roi_encoder as RE
    from oracle.roi_align import assign_boxes_to_levels
    from sylph_amd import synthetic as W
    feats, boxes, roi_image, seg_len = _toy()
    assert sorted(set(assign_boxes_to_levels(boxes, 3, 4).tolist())) == [0, 1]  # both levels are read
    strides = (8, 16)
    if kind == "roienc":
        sd, kw = W.roi_encoder_state_dict(seed=4), {}
    else:
        w = kind == "weighted"
        sd = W.codegen_state_dict(seed=2, weight_scale_layers=w)
        kw = dict(has_weight_layer=w, has_scale_layer=w, bias_l2_norm=w)
    got = segment_code_dicts(kind, feats, boxes, roi_image, seg_len, sd, strides=strides, **kw)
    packed = segment_codes(kind, feats, boxes, roi_image, seg_len, sd, strides=strides, **kw)
    assert len(got) == 2 and tuple(packed.shape) == (2, 257)
    r0 = 0
    for j, n in enumerate(seg_len):
        dup = [torch.stack([f[roi_image[r]] for r in range(r0, r0 + n)]) for f in feats]
        bx = torch.stack([boxes[r] for r in range(r0, r0 + n)])
        if kind == "roienc":
            want = RE.roi_encoder(dup, bx, sd, num_shots=n, strides=strides)
        else:
            want = CG.code_generator(dup, bx, sd, strides=strides, **kw)
        assert set(got[j]) == set(want)
        for k in want:
            assert torch.equal(got[j][k], want[k]), (kind, j, k)
        assert torch.equal(packed[j], torch.cat([want["cls_conv"].reshape(-1), want["cls_bias"].reshape(-1)]))
        r0 += n
    # segments never see each other: a segment alone gives the same code as inside the list
    alone = segment_codes(kind, feats, boxes[2:], roi_image[2:], [3], sd, strides=strides, **kw)
    assert torch.equal(alone[0], packed[1])


# ------------------------------------------------------------------------------------------------ C ABI
def test_roi_list_symbols_declared_and_exported():
    from sylph_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sylph_hip.h")).read()
    declared = set(re.findall(r"\b(sylph_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in ("sylph_codegen_rois", "sylph_roi_align_rois"):
        assert name in declared and name in _lib.PROTOTYPES
        assert getattr(L, name) is not None
    assert len(_lib.PROTOTYPES["sylph_codegen_rois"][1]) == 7 and len(_lib.PROTOTYPES["sylph_roi_align_rois"][1]) == 5


def test_model_rejects_bad_segments_before_any_device_work():
    """forward_class_codes_rois validates its segments on the host, before the backbone runs."""
    from sylph_amd.modeling import MetaOneStageDetector

    class Stub:
        training = False
        episodic_learning = True
        code_generator = type("G", (), {"forward_rois": None})()

        def backbone(self, images):
            raise AssertionError("the backbone must not run for an invalid segment list")

    recs = [{"image": torch.zeros(3, 32, 32)}] * 2
    f = MetaOneStageDetector.forward_class_codes_rois
    with pytest.raises(ValueError, match="segment 1 is empty"):
        f(Stub(), recs, [{"image_index": torch.tensor([0]), "boxes": torch.zeros(1, 4)},
                         {"image_index": torch.zeros(0, dtype=torch.long), "boxes": torch.zeros(0, 4)}])
    with pytest.raises(ValueError, match="image_index 2"):
        f(Stub(), recs, [{"image_index": torch.tensor([2]), "boxes": torch.zeros(1, 4)}])
    with pytest.raises(ValueError):
        f(Stub(), recs, [])


def test_roi_encoder_forward_rois_needs_eval_shot_segments():
    """ROIEncoder.forward_rois asserts EVAL_SHOT ROIs per segment, as forward_classes does for its shots, before any engine call."""
    from sylph_amd.config import get_default_cfg
    from sylph_amd.modeling import ROIEncoder
    cfg = get_default_cfg()
    cfg.MODEL.META_LEARN.EVAL_SHOT = 5
    enc = ROIEncoder(cfg)
    assert enc.engine is None  # an engine call would fail on None: the assertion must come first
    with pytest.raises(AssertionError, match="segment 1 has 3 ROIs, EVAL_SHOT is 5"):
        enc.forward_rois(torch.zeros(8, 4), [0] * 8, [5, 3])
