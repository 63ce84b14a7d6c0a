"""Query views on the GPU: sylph_preprocess_views against Pillow, sylph_merge_views against the float32 numpy reference
(tests/views_ref.py), and the model's views path (TEST.AUG, tiles) against the composition of the existing paths: host-made views
through preprocess_u8, decode at the crop size, the numpy merge.  Every comparison is exact (torch.equal / array_equal)."""
import numpy as np
import pytest
import torch

import views_ref as VR
from test_hip_parity import _cfg
from test_views_cpu import MERGE_COUNTS, interleaved_table

pytestmark = pytest.mark.gpu

MEAN, STD = [103.530, 116.280, 123.675], [1.0, 1.0, 1.0]
LOW_TH = {"MODEL.FCOS.INFERENCE_TH_TEST": 0.02}  # detections exist on small synthetic-weight views


@pytest.fixture(scope="module")
def sd():
    from sylph_amd import synthetic as W
    return W.synthetic_state_dict(0, depth=50)


def _u8(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def _engine(dtype, sd, **over):
    from sylph_amd.engine import Engine
    eng = Engine(_cfg(**over), dtype=dtype)
    if sd is not None:
        eng.load_state_dict(sd)
    return eng


def _codes(n, seed):
    from sylph_amd import synthetic as W
    return {k: v.cuda() for k, v in W.synthetic_codes(n, seed=seed, scale=3.0).items()}


# ------------------------------------------------------------------------------------------------ 1: the input kernel against Pillow
def _input_views():
    """(source index, view): sources 0 = 37 x 53, 1 = 64 x 48 (h x w); every view also mirrored"""
    from sylph_amd.views import make_view
    base = [(0, make_view((0, 0, 53, 37), (37, 53))),      # the full frame at its own size
            (1, make_view((5, 7, 29, 31), (44, 40))),      # a crop, upscaled
            (1, make_view((3, 2, 43, 60), (22, 16))),      # shrunk by 2.73 / 2.69: filter support above one pixel
            (0, make_view((20, 10, 33, 27), (30, 30))),    # touches the right and the bottom edge
            (0, make_view((10, 5, 2, 20), (20, 5)))]       # 2 pixels wide
    out = []
    for s, v in base:
        out.append(dict(v, source=s))
        out.append(dict(v, source=s, flip=True))
    return out


@pytest.mark.parametrize("dtype", ["f32", "f32s", "bf16"])
def test_preprocess_views_against_pillow(dtype, sd):
    srcs = [_u8(37, 53, 1), _u8(64, 48, 2)]
    views = _input_views()
    eng = _engine(dtype, sd)
    dev = [torch.from_numpy(s).cuda() for s in srcs]
    for rgb in (False, True):
        ph, pw = eng.preprocess_views(dev, views, rgb_input=rgb)
        got = eng.export_input().cpu().numpy()
        want = VR.network_input([VR.view_image(srcs[v["source"]], v) for v in views], MEAN, STD, rgb)
        assert (ph, pw) == want.shape[2:] == (64, 64)
        if dtype == "bf16":
            want = VR.bf16_round(want)
        assert np.array_equal(got, want), f"{dtype}, rgb_input={rgb}: {np.argwhere(got != want)[:4].tolist()}"
        for b, v in enumerate(views):  # padding zeros included
            assert np.all(got[b, :, v["size"][0]:] == 0) and np.all(got[b, :, :, v["size"][1]:] == 0)
        # the full-frame, unflipped view is what preprocess_u8 gives the source itself
        eng.preprocess_views(dev, views[:1], rgb_input=rgb)
        one = eng.export_input()
        eng.preprocess_u8([dev[0]], [(37, 53)], rgb_input=rgb)
        assert torch.equal(one, eng.export_input())
    eng.close()


def test_preprocess_views_refusals(sd):
    eng = _engine("bf16", sd)
    src = [torch.from_numpy(_u8(37, 53, 1)).cuda()]
    for crop, size in (((30, 0, 29, 10), (10, 10)), ((0, 30, 10, 8), (10, 10)), ((-1, 0, 10, 10), (10, 10))):
        with pytest.raises(RuntimeError, match="leaves its"):
            eng.preprocess_views(src, [{"source": 0, "crop": crop, "size": size, "flip": False}])
    for crop, size in (((0, 0, 0, 10), (10, 10)), ((0, 0, 10, 10), (0, 10))):
        with pytest.raises(RuntimeError, match="non-positive"):
            eng.preprocess_views(src, [{"source": 0, "crop": crop, "size": size, "flip": False}])
    eng.close()


# ------------------------------------------------------------------------------------------------ 2: the merge kernel on synthetic rows
def _rows(boxes, scores, classes, counts):
    return {"boxes": torch.from_numpy(boxes).cuda(), "scores": torch.from_numpy(scores).cuda(), "classes": torch.from_numpy(classes).cuda(),
            "counts": torch.from_numpy(counts).cuda()}


def _assert_merged(got, want, what):
    for s, (g, w) in enumerate(zip(got, want)):
        assert g["scores"].numel() == len(w["scores"]), f"{what}: source {s}: {g['scores'].numel()} rows, expected {len(w['scores'])}"
        for k in ("scores", "pred_boxes", "pred_classes", "view_index", "view_row"):
            assert torch.equal(g[k].cpu(), torch.from_numpy(w[k])), f"{what}: source {s}: {k} differs"


@pytest.fixture(scope="module")
def small_case():
    table = interleaved_table()
    return (table,) + VR.draw_rows(table, 16, MERGE_COUNTS, 3, seed=11, thr=0.6, score_levels=12)


def test_merge_views_interleaved_sources(small_case):
    """3 sources with 1, 4 and 7 views, interleaved; counts 0 ... 16 of max_in 16; flips, offsets, equal scores across views"""
    table, boxes, scores, classes, counts = small_case
    full = VR.merge_ref(table, boxes, scores, classes, counts, 3, 0.6, 0)
    ties = [k for k in range(1, len(full[2]["scores"])) if full[2]["scores"][k] == full[2]["scores"][k - 1]]
    assert ties, "no K-th-place tie in the drawn data"
    for thr, K in ((0.6, 100), (0.6, ties[0]), (0.6, 0), (0.0, 0), (0.0, 7)):
        eng = _engine("bf16", None, **{"MODEL.FCOS.NMS_TH": thr, "MODEL.FCOS.POST_NMS_TOPK_TEST": K})
        want = VR.merge_ref(table, boxes, scores, classes, counts, 3, thr, K)
        if (thr, K) == (0.6, ties[0]):
            assert len(want[2]["scores"]) > K, "the tie at the K-th place is kept"
        if thr == 0.0 and K == 0:  # NMS off: everything, in stable score order
            assert [len(w["scores"]) for w in want] == [sum(c for c, t in zip(MERGE_COUNTS, table) if t["source"] == s) for s in range(3)]
        _assert_merged(eng.merge_views(table, _rows(boxes, scores, classes, counts), max_out=200), want, f"NMS_TH {thr}, K {K}")
        eng.close()


def test_merge_views_truncation_sets_status(small_case):
    table, boxes, scores, classes, counts = small_case
    eng = _engine("bf16", None, **{"MODEL.FCOS.NMS_TH": 0.0, "MODEL.FCOS.POST_NMS_TOPK_TEST": 0})
    with pytest.raises(RuntimeError, match="max_out"):
        eng.merge_views(table, _rows(boxes, scores, classes, counts), max_out=20)  # source 2 holds 68 rows
    # the call after it starts from a clear status word
    want = VR.merge_ref(table, boxes, scores, classes, counts, 3, 0.0, 0)
    _assert_merged(eng.merge_views(table, _rows(boxes, scores, classes, counts), max_out=200), want, "after a truncated call")
    eng.close()


def test_merge_views_1280_rows_of_one_source():
    """20 views x 64 rows: the pool passes one 64-box chunk, passes 1024 and is not a power of two; a second source holds 3 rows"""
    table = [{"source": 0, "crop": (3 * (v % 5), 2 * (v % 3), 250, 200), "flip": v % 2 == 1} for v in range(20)]
    table.insert(7, {"source": 1, "crop": (0, 0, 250, 200), "flip": False})
    counts = [64] * 21
    counts[7] = 3
    boxes, scores, classes, cnt = VR.draw_rows(table, 64, counts, 4, seed=5, thr=0.6, score_levels=0, n_objects=60)
    for K in (0, 100):
        eng = _engine("bf16", None, **{"MODEL.FCOS.NMS_TH": 0.6, "MODEL.FCOS.POST_NMS_TOPK_TEST": K})
        want = VR.merge_ref(table, boxes, scores, classes, cnt, 2, 0.6, K)
        if K == 0:
            assert len(want[0]["scores"]) > 64, "the kept list itself crosses a chunk"
        _assert_merged(eng.merge_views(table, _rows(boxes, scores, classes, cnt), max_out=1280), want, f"1280 rows, K {K}")
        eng.close()


def test_merge_views_pool_above_capacity_fails_by_name():
    from sylph_amd.engine import _iarr, _ptr
    import ctypes
    eng = _engine("bf16", None)
    nv, max_in, max_out = 65, 64, 8  # 4160 rows > MERGE_POOL_CAP
    z = lambda *s, dt=torch.float32: torch.zeros(*s, device="cuda", dtype=dt)
    fa = (ctypes.c_float * nv)(*([0.0] * nv))
    outs = [torch.full((max_out * 4,), -7.0, device="cuda"), torch.full((max_out,), -7.0, device="cuda")] + \
           [torch.full((max_out,), -7, device="cuda", dtype=torch.int32) for _ in range(5)]
    rc = eng.L.sylph_merge_views(eng._ctx, 1, nv, _iarr([0] * nv), fa, fa, fa, _iarr([0] * nv), max_in, _ptr(z(nv, max_in, 4)), _ptr(z(nv, max_in)),
                                 _ptr(z(nv, max_in, dt=torch.int32)), _ptr(z(nv, dt=torch.int32)), max_out, *[_ptr(t) for t in outs[:6]], _ptr(outs[6]))
    assert rc != 0 and b"MERGE_POOL_CAP" in eng.L.sylph_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in outs), "a refused call writes nothing"
    with pytest.raises(RuntimeError, match="MERGE_POOL_CAP"):
        eng.merge_views([{"source": 0, "crop": (0, 0, 10, 10), "flip": False}] * nv,
                        {"boxes": z(nv, max_in, 4), "scores": z(nv, max_in), "classes": z(nv, max_in, dt=torch.int32), "counts": z(nv, dt=torch.int32)})
    eng.close()


# ------------------------------------------------------------------------------------------------ 3: identity
def test_one_full_frame_view_per_source_is_decode(sd):
    """Decode runs its NMS on the unclipped boxes and clips them to the output size afterwards; the merge sees the clipped rows.  A row
    that the clip shortened can overlap a neighbour more than it did under decode's NMS (with the synthetic weights' regression as it
    is, a 96 x 128 image gives 97 rows of which the merge keeps 74), so the identity is one of UNCLIPPED rows.  The images fill their
    padded size (no location lies outside an image) and the real head's regression goes back in clamped to 0.45 strides
    (export_head -> import_head): every box then lies strictly inside its image, which the test asserts."""
    eng = _engine("bf16", sd, **LOW_TH)
    srcs = [torch.from_numpy(_u8(128, 128, 21)).cuda(), torch.from_numpy(_u8(128, 128, 22)).cuda()]
    sizes = [(128, 128), (128, 128)]
    c = _codes(5, 42)
    eng.preprocess_u8(srcs, sizes)
    eng.backbone()
    eng.head(c["cls_conv"], c["cls_bias"])
    lo, rg, ct, io = eng.export_head()
    eng.import_head(lo, [r.clamp(max=0.45) for r in rg], ct, io)
    want = eng.decode(sizes)
    assert all(d["scores"].numel() > 0 for d in want), "no detections: the comparison proves nothing"
    for d, (h, w) in zip(want, sizes):
        b = d["pred_boxes"]
        assert bool((b[:, :2] > 0).all()) and bool((b[:, 2] < w).all()) and bool((b[:, 3] < h).all()), "a row was clipped"
    table = [{"source": i, "crop": (0, 0, s[1], s[0]), "size": s, "flip": False} for i, s in enumerate(sizes)]
    rows = eng.new_view_rows(2)
    eng.decode_rows(rows, 0, sizes)
    got = eng.merge_views(table, rows)
    for i, (g, w) in enumerate(zip(got, want)):
        n = w["scores"].numel()
        assert g["scores"].numel() == n
        assert torch.equal(g["pred_boxes"], w["pred_boxes"]) and torch.equal(g["scores"], w["scores"])
        assert torch.equal(g["pred_classes"], w["pred_classes"])
        assert torch.equal(g["view_index"].cpu(), torch.full((n,), i)) and torch.equal(g["view_row"].cpu(), torch.arange(n))
    eng.close()


# ------------------------------------------------------------------------------------------------ 4 + 5: the model against the composition
def _model(dtype, sd, **over):
    from sylph_amd.modeling import MetaOneStageDetector
    cfg = _cfg(**dict(LOW_TH, **over))
    m = MetaOneStageDetector(cfg, dtype=dtype)
    m.load_state_dict(sd)
    m.eval()
    return m


def _composition(model, srcs, per_input_views, codes):
    """The same step batches from host-made views through preprocess_u8, decode at the crop sizes, then the numpy merge -> per input
    the merged dict with view_index mapped to the input's own view list.  codes: a dict, or one dict per input."""
    from sylph_amd.modeling import group_episodes
    from sylph_amd.views import plan_view_steps, view_out_size
    eng = model.engine
    table = [dict(v, source=i, view=k) for i, vs in enumerate(per_input_views) for k, v in enumerate(vs)]
    steps = plan_view_steps(table, model.view_max_batch)
    table = [table[i] for st in steps for i in st]
    m = eng.default_max_out()
    V = len(table)
    boxes, scores = np.zeros((V, m, 4), np.float32), np.zeros((V, m), np.float32)
    classes, counts = np.zeros((V, m), np.int32), np.zeros(V, np.int32)
    row0 = 0
    for st in steps:
        vs = table[row0:row0 + len(st)]
        imgs = [torch.from_numpy(VR.view_image(srcs[v["source"]], v).copy()).cuda() for v in vs]
        eng.preprocess_u8(imgs, [v["size"] for v in vs])
        eng.backbone()
        if isinstance(codes, list):
            dicts, ep = group_episodes(codes, len(srcs))
            eng.head_episodes([(d["cls_conv"], d["cls_bias"]) for d in dicts], [ep[v["source"]] for v in vs])
        else:
            eng.head(codes["cls_conv"], codes["cls_bias"])
        for k, d in enumerate(eng.decode([view_out_size(v) for v in vs])):
            n = d["scores"].numel()
            counts[row0 + k] = n
            boxes[row0 + k, :n] = d["pred_boxes"].cpu().numpy()
            scores[row0 + k, :n] = d["scores"].cpu().numpy()
            classes[row0 + k, :n] = d["pred_classes"].cpu().numpy()
        row0 += len(st)
    assert counts.sum() > 0 and (counts > 0).sum() >= V // 2, f"too few views with detections: {counts.tolist()}"
    merged = VR.merge_ref(table, boxes, scores, classes, counts, len(srcs), float(model.cfg.MODEL.FCOS.NMS_TH),
                          int(model.cfg.MODEL.FCOS.POST_NMS_TOPK_TEST))
    own = np.array([v["view"] for v in table])
    for d in merged:
        d["view_index"] = own[d["view_index"]]
    return merged


def _assert_model(got, want, srcs):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        r = g["instances"]
        assert r.image_size == srcs[i].shape[:2]
        assert len(r) == len(w["scores"]) > 0, (i, len(r), len(w["scores"]))
        assert torch.equal(r.scores.cpu(), torch.from_numpy(w["scores"])), f"input {i}: scores"
        assert torch.equal(r.pred_boxes.tensor.cpu(), torch.from_numpy(w["pred_boxes"])), f"input {i}: boxes"
        assert torch.equal(r.pred_classes.cpu(), torch.from_numpy(w["pred_classes"])), f"input {i}: classes"
        assert torch.equal(r.view_index.cpu(), torch.from_numpy(w["view_index"])), f"input {i}: view_index"
        assert torch.equal(r.view_row.cpu(), torch.from_numpy(w["view_row"])), f"input {i}: view_row"


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_model_tta_equals_composition(dtype, sd):
    from sylph_amd.views import tta_views
    aug = {"TEST.AUG.ENABLED": True, "TEST.AUG.MIN_SIZES": (64, 96), "TEST.AUG.MAX_SIZE": 160, "TEST.AUG.FLIP": True}
    model = _model(dtype, sd, **aug)
    srcs = [_u8(96, 128, 31), _u8(120, 90, 32)]
    batch = [{"image_u8": torch.from_numpy(s), "resize_hw": s.shape[:2]} for s in srcs]
    views = [tta_views(s.shape[0], s.shape[1], (64, 96), 160, True) for s in srcs]
    assert [len(v) for v in views] == [4, 4]
    d0, d1 = _codes(5, 42), _codes(5, 45)
    kw = dict(run_type="meta_learn_test_instance")
    for codes in (d0, [d0, d1]):  # a uniform code; per-input codes (the mixed-episode head: all views of an input take its episode)
        got = model(batch, class_code=codes, **kw)
        _assert_model(got, _composition(model, srcs, views, codes), srcs)
    # explicit views win over TEST.AUG, and "height" / "width" rescale as detector_postprocess does
    got = model([dict(batch[0], views=views[0][:2], height=48, width=64)], class_code=d0, **kw)[0]["instances"]
    want = _composition(model, srcs[:1], [views[0][:2]], d0)[0]
    assert got.image_size == (48, 64) and len(got) > 0
    wb = torch.from_numpy(want["pred_boxes"]) * torch.tensor([0.5, 0.5, 0.5, 0.5])
    wb = torch.minimum(wb.clamp(min=0), torch.tensor([64.0, 48.0, 64.0, 48.0]))
    keep = ((wb[:, 2] - wb[:, 0]) > 0) & ((wb[:, 3] - wb[:, 1]) > 0)
    assert torch.equal(got.pred_boxes.tensor.cpu(), wb[keep]) and torch.equal(got.scores.cpu(), torch.from_numpy(want["scores"])[keep])


def test_model_tiles_equal_composition(sd):
    from sylph_amd.views import tile_views
    model = _model("bf16", sd)
    srcs = [_u8(150, 200, 41)]
    views = [tile_views(150, 200, (96, 96), 0.25, 96, 160)]
    assert len(views[0]) == 7  # the full frame + 2 x 3 tiles
    d0 = _codes(5, 42)
    batch = [{"image_u8": torch.from_numpy(srcs[0]), "resize_hw": (96, 128), "views": views[0]}]
    got = model(batch, class_code=d0, run_type="meta_learn_test_instance")
    _assert_model(got, _composition(model, srcs, views, d0), srcs)
    assert len(set(got[0]["instances"].view_index.tolist())) > 1, "detections of one view only"


def test_box_across_tile_borders_comes_out_once(sd):
    """A box planted through import_head in the four tiles that see it whole: one detection in source pixels."""
    from sylph_amd.views import tile_views
    eng = _engine("f32", sd)
    views = tile_views(150, 200, (96, 96), 0.25, None, 4000, full_frame=False)
    assert [v["crop"][:2] for v in views] == [(0, 0), (72, 0), (104, 0), (0, 54), (72, 54), (104, 54)]
    box, cls = (74.0, 60.0, 94.0, 90.0), 2  # inside the 24-pixel overlap of columns 0 / 1 and the 42-pixel overlap of the rows
    shapes = eng.level_shapes(96, 96)
    eng.import_pyramid([torch.zeros(6, 256, h, w) for h, w in shapes], (96, 96), [(96, 96)] * 6)
    logits = [torch.full((6, 3, h, w), -20.0) for h, w in shapes]
    reg = [torch.zeros(6, 4, h, w) for h, w in shapes]
    ctr = [torch.full((6, 1, h, w), 10.0) for h, w in shapes]
    seen = []
    for b, v in enumerate(views):
        x0, y0 = v["crop"][:2]
        bx = (box[0] - x0, box[1] - y0, box[2] - x0, box[3] - y0)
        if bx[0] < 0 or bx[1] < 0 or bx[2] > 96 or bx[3] > 96:
            continue
        lx, ly = int((bx[0] + bx[2]) / 2) // 8, int((bx[1] + bx[3]) / 2) // 8  # a P3 location inside the box
        x, y = lx * 8 + 4, ly * 8 + 4
        assert bx[0] <= x <= bx[2] and bx[1] <= y <= bx[3]
        logits[0][b, cls, ly, lx] = 4.0 + 0.25 * b  # the views disagree on the score
        reg[0][b, :, ly, lx] = torch.tensor([x - bx[0], y - bx[1], bx[2] - x, bx[3] - y]) / 8.0
        seen.append(b)
    assert seen == [0, 1, 3, 4]
    eng.import_head(logits, reg, ctr)
    rows = eng.new_view_rows(6)
    eng.decode_rows(rows, 0, [(96, 96)] * 6)
    assert rows["counts"].tolist() == [1, 1, 0, 1, 1, 0]
    out = eng.merge_views([dict(v, source=0) for v in views], rows)[0]
    assert out["scores"].numel() == 1
    assert out["pred_boxes"].cpu().tolist() == [list(box)] and out["pred_classes"].tolist() == [cls]
    assert out["view_index"].tolist() == [4] and out["view_row"].tolist() == [0]  # the best-scored copy
    eng.close()


# ------------------------------------------------------------------------------------------------ 6: refusals
def test_model_refusals(sd):
    from sylph_amd.views import make_view
    model = _model("bf16", sd)
    src = torch.from_numpy(_u8(96, 128, 31))
    d0 = _codes(5, 42)
    kw = dict(run_type="meta_learn_test_instance")
    views = [make_view((0, 0, 128, 96), (64, 85))]
    with pytest.raises(NotImplementedError, match="class_code_sets"):
        model([{"image_u8": src, "resize_hw": (96, 128), "views": views}], class_code_sets=[d0, d0], **kw)
    with pytest.raises(ValueError, match="leaves its"):
        model([{"image_u8": src, "resize_hw": (96, 128), "views": [make_view((100, 0, 64, 64), (64, 64))]}], class_code=d0, **kw)
    model.cfg.TEST.AUG.ENABLED = True
    with pytest.raises(ValueError, match="TEST.AUG.ENABLED"):
        model([{"image": torch.zeros(3, 96, 128)}], class_code=d0, **kw)
    model.cfg.TEST.AUG.ENABLED = False
    # without views and with TEST.AUG off nothing changes: the plain path
    plain = model([{"image_u8": src, "resize_hw": (96, 128)}], class_code=d0, **kw)[0]["instances"]
    assert plain.has("locations") and not plain.has("view_index")
