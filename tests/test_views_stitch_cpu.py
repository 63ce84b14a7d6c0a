"""The stitching view merge, host side (no GPU): the numpy reference of tests/views_stitch_ref.py against the large merge's where no
row is cut, on tiled scenes where it has to return every object once and whole, under mirrored views; rule 0's host helper; the C
ABI's declarations; the workspace size; the route.  tests/test_views_stitch_gpu.py takes its scenes from here."""
import functools
import os
import re

import numpy as np
import pytest

import views_large_ref as LR
import views_stitch_ref as SR
from sylph_amd import views as V
from test_views_large_cpu import pool_4300

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("pred_boxes", "scores", "pred_classes", "view_index", "view_row")
# the two scenes of a 3000 x 4000 source under 800-pixel tiles, overlap 0.2, full frame first: object sides, objects asked for, the
# full frame's score range (low: the tiles' fragments come first in rule-3 order; wide: the full frame's whole box often does)
SCENES = {"40-420 px": (40, 420, 60, (0.25, 0.1)), "300-1300 px": (300, 1300, 25, (0.25, 0.5))}


@functools.lru_cache(maxsize=None)
def scene(name, seed, flipped=()):
    lo, hi, n_obj, full_score = SCENES[name]
    return SR.tiled_scene(seed, lo, hi, n_obj, full_score, flipped=flipped)


@pytest.mark.parametrize("thr,K", [(0.6, 100), (0.6, 0), (0.0, 100), (0.6, 7)])
def test_without_cut_rows_it_is_the_large_merge(thr, K):
    table, boxes, scores, classes, counts = pool_4300()
    a = SR.stitch_ref(table, boxes, scores, classes, counts, 1, [(400, 400)], thr, K, no_cut=True)[0]
    b = LR.merge_large_ref(table, boxes, scores, classes, counts, 1, thr, K)[0]
    for key in KEYS:
        assert np.array_equal(a[key], b[key]), key
    assert a["kept"] == b["kept"] and a["absorbed"] == a["dropped"] == 0
    assert (a["stitched"] == 1).all() and len(a["stitched"]) == len(a["scores"])
    if thr > 0:
        assert a["suppressed"] > 0, "NMS has work"
    # the same pool under rule 0: rows that leave their crop on the left or the top are cut, and the result is another one
    c = SR.stitch_ref(table, boxes, scores, classes, counts, 1, [(400, 400)], thr, K)[0]
    assert c["cut_rows"] > 0 and c["absorbed"] > 0 and not np.array_equal(c["view_row"], b["view_row"])


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("name", list(SCENES))
def test_every_object_comes_back_once_and_whole(name, seed):
    """What the feature is for: every view returns ground truth clipped to its crop; the plain merge keeps the pieces, the stitching
    merge returns exactly one box per object, equal to its ground-truth box."""
    pool, gt, hw = scene(name, seed)
    ref = SR.assert_margins(pool, 1, [hw], 0.6)[0]
    assert ref["cut_rows"] > 0 and ref["absorbed"] > 0 and ref["suppressed"] > 0
    if name == "300-1300 px":
        assert ref["dropped"] > 0, "rule 4b has work: a fragment kept before the row that bridges it to its object"
    assert len(ref["scores"]) == len(gt)
    got = {tuple(b) for b in ref["pred_boxes"].tolist()}
    assert got == {tuple(g) for g in gt.tolist()} and len(got) == len(gt)
    total = int(ref["stitched"].sum())  # every cut-pair absorption and every drop counts once; what a dropped row had absorbed is not passed on
    assert len(gt) + ref["dropped"] < total <= len(gt) + ref["absorbed"] + ref["dropped"]
    if ref["dropped"] == 0:
        assert total == len(gt) + ref["absorbed"]
    plain = LR.merge_large_ref(*pool, 1, 0.6, 0)[0]
    assert len(plain["scores"]) > len(gt), "the plain merge keeps the pieces"


def test_mirroring_views_changes_nothing():
    pool, gt, hw = scene("300-1300 px", 1)
    flipped = tuple(range(0, len(pool[0]), 3))  # the full frame and every third tile
    mirrored = scene("300-1300 px", 1, flipped)[0]
    assert [t["flip"] for t in mirrored[0]] != [t["flip"] for t in pool[0]] and not np.array_equal(mirrored[1], pool[1])
    a = SR.stitch_ref(*pool, 1, [hw], 0.6, 0)[0]
    b = SR.stitch_ref(*mirrored, 1, [hw], 0.6, 0)[0]
    for key in KEYS + ("stitched",):
        assert np.array_equal(a[key], b[key]), key
    assert a["cut_rows"] == b["cut_rows"] > 0


def test_cut_flags():
    view = {"crop": (100, 200, 300, 400)}  # L 100, T 200, R 400, B 600
    hw = (1000, 1000)
    inside = [150.0, 250.0, 350.0, 550.0]
    cases = {"inside": (inside, False), "left": ([100, 250, 350, 550], True), "right": ([150, 250, 400, 550], True),
             "top": ([150, 200, 350, 550], True), "bottom": ([150, 250, 350, 600], True), "top-left": ([100, 200, 350, 550], True),
             "bottom-right": ([150, 250, 400, 600], True), "top-right": ([150, 200, 400, 550], True), "bottom-left": ([100, 250, 350, 600], True),
             "two pixels from the left": ([102, 250, 350, 550], True), "2.5 pixels from the left": ([102.5, 250, 350, 550], False),
             "two pixels from the bottom": ([150, 250, 350, 598], True), "2.5 pixels from the right": ([150, 250, 397.5, 550], False)}
    boxes = np.array([c[0] for c in cases.values()], dtype=np.float32)
    got = V.cut_flags(view, hw, boxes, 2.0)
    assert got.dtype == bool and got.tolist() == [c[1] for c in cases.values()], dict(zip(cases, got.tolist()))
    # border_px 0: only a box that reaches the border itself
    zero = V.cut_flags(view, hw, boxes, 0.0)
    want0 = [c[1] and "pixels" not in k for k, c in cases.items()]
    assert zero.tolist() == want0
    # a crop border that is the source's own never cuts
    assert not V.cut_flags({"crop": (0, 0, 400, 600)}, (600, 400), boxes, 2.0).any()
    full = np.array([[0, 0, 400, 600], [0, 0, 10, 10], [390, 590, 400, 600]], dtype=np.float32)
    assert not V.cut_flags({"crop": (0, 0, 400, 600)}, (600, 400), full, 2.0).any()
    # ... side by side: a crop in the source's top-left corner cuts on the right and at the bottom only
    corner = {"crop": (0, 0, 400, 600)}
    assert V.cut_flags(corner, hw, full, 2.0).tolist() == [True, False, True]
    assert V.cut_flags(corner, (600, 1000), full, 2.0).tolist() == [True, False, True]  # (the right border still cuts)
    assert V.cut_flags(corner, (600, 1000), np.array([[0, 590, 10, 600]], np.float32), 2.0).tolist() == [False]
    assert V.cut_flags(view, hw, np.zeros((0, 4), np.float32), 2.0).shape == (0,)


def test_header_and_library_agree_on_the_stitching_merge():
    from sylph_amd import _lib
    text = open(os.path.join(ROOT, "include", "sylph_hip.h")).read()
    for ret, name, nargs in (("int64_t", "sylph_stitch_views_bytes", 3), ("int", "sylph_stitch_views", 30)):
        m = re.search(ret + r"\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"include/sylph_hip.h does not declare {name}"
        assert len(m.group(1).split(",")) == nargs
        assert len(_lib.PROTOTYPES[name][1]) == nargs
        assert hasattr(_lib.lib(), name)
    for word in ("view_h", "src_w", "src_h", "stitch_thr", "border_px", "out_stitched_dev"):
        assert word in m.group(1)
    assert "sylph_stitch_views (below) joins them" in text  # the caveat above sylph_merge_views points here


def test_workspace_size_function():
    from sylph_amd import _lib
    L = _lib.lib()
    last = 0
    for n_src, nv, max_in in ((1, 1, 1), (1, 1, 2048), (1, 1, 2049), (1, 21, 200), (3, 150, 100), (3, 209, 200), (8, 5243, 200)):
        need = L.sylph_stitch_views_bytes(n_src, nv, max_in)
        assert need >= L.sylph_merge_views_large_bytes(n_src, nv, max_in) > 0
        assert need >= last
        last = need
    assert L.sylph_stitch_views_bytes(1, 1 << 20, 1 << 11) == -1 and b"row index" in L.sylph_last_error()  # 2^31 rows
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        assert L.sylph_stitch_views_bytes(*bad) == -1 and b"sylph_stitch_views_bytes" in L.sylph_last_error()


def test_route_and_parameters():
    assert V.stitch_params(None) is None and V.stitch_params(False) is None
    assert V.stitch_params(True) == (0.5, 2.0) == (V.DEFAULT_STITCH_THR, V.DEFAULT_STITCH_BORDER)
    assert V.stitch_params({"thr": 0.7}) == (0.7, 2.0) and V.stitch_params({"border": 0}) == (0.5, 0.0)
    assert V.stitch_params({"thr": 1.0, "border": 3.5}) == (1.0, 3.5)
    for bad, match in (({"thr": 0.0}, "thr"), ({"thr": 1.5}, "thr"), ({"thr": float("nan")}, "thr"), ({"border": -1}, "border"),
                       ({"border": float("nan")}, "border"), ({"threshold": 0.5}, "stitch"), ("yes", "stitch")):
        with pytest.raises(ValueError, match=match):
            V.stitch_params(bad)
    # without stitching the route is merge_route's, unchanged
    for per_source, max_in, topk in (([20], 200, None), ([21], 200, None), ([7, 21, 1], 200, None), ([], 200, None), ([1], 200, 100)):
        assert V.view_merge_route(per_source, max_in, topk, None) == V.merge_route(per_source, max_in, topk)
        assert V.view_merge_route(per_source, max_in, topk, (0.5, 2.0)) == "stitch"
