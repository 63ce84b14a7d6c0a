"""The large view merge, host side (no GPU): the greedy numpy reference of tests/views_large_ref.py against the two references of
tests/views_ref.py, the router between the two merges, the C ABI's declarations, and the view count that makes the large merge
necessary.  tests/test_views_large_gpu.py takes its drawn pools from here."""
import functools
import os
import re

import numpy as np
import pytest

import views_large_ref as LR
import views_ref as VR
from sylph_amd import views as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("pred_boxes", "scores", "pred_classes", "view_index", "view_row")


def one_source_table(n_views, source=0):
    """views of one 250 x 200 source region with small offsets, every second one mirrored"""
    return [{"source": source, "crop": (3 * (v % 5), 2 * (v % 3), 250, 200), "flip": v % 2 == 1} for v in range(n_views)]


@functools.lru_cache(maxsize=None)
def drawn_pool(n_views, max_in, n_classes, seed, score_levels=0, n_objects=60, n_src=1):
    """(table, boxes, scores, classes, counts) of n_views full views, view v belonging to source v % n_src; drawn once per process
    (draw_rows enforces and asserts the 1e-4 IoU margin from NMS_TH 0.6)"""
    table = [dict(t, source=v % n_src) for v, t in enumerate(one_source_table(n_views))]
    return (table,) + VR.draw_rows(table, max_in, [max_in] * n_views, n_classes, seed=seed, thr=0.6, score_levels=score_levels,
                                   n_objects=n_objects)


def pool_4300():
    """43 views x 100 rows of one source, 5 classes, scores quantised to 40 levels: ties at the K-th place"""
    return drawn_pool(43, 100, 5, 7, score_levels=40)


@pytest.mark.parametrize("thr,K", [(0.6, 100), (0.6, 0), (0.0, 100)])
def test_three_references_agree(thr, K):
    table, boxes, scores, classes, counts = pool_4300()
    a = LR.merge_large_ref(table, boxes, scores, classes, counts, 1, thr, K)
    b = VR.merge_ref(table, boxes, scores, classes, counts, 1, thr, K)
    c = VR.merge_bruteforce(table, boxes, scores, classes, counts, 1, thr, K)
    for key in KEYS:
        assert np.array_equal(a[0][key], b[0][key]), ("merge_ref", key)
        assert np.array_equal(a[0][key], c[0][key]), ("merge_bruteforce", key)
    if thr > 0:
        assert a[0]["kept"] < 4300, "NMS has work"
    if K > 0:
        assert a[0]["kept"] > K and len(a[0]["scores"]) > K, "rule 5 cuts, and the K-th score is tied"


def test_reference_clamps_counts_and_truncates():
    table, boxes, scores, classes, counts = pool_4300()
    wild = counts.copy()
    wild[0], wild[1] = 100 + 37, -5
    clamped = counts.copy()
    clamped[1] = 0
    a = LR.merge_large_ref(table, boxes, scores, classes, wild, 1, 0.6, 0)
    b = LR.merge_large_ref(table, boxes, scores, classes, clamped, 1, 0.6, 0)
    for key in KEYS:
        assert np.array_equal(a[0][key], b[0][key])
    cut = LR.merge_large_ref(table, boxes, scores, classes, counts, 1, 0.6, 0, max_out=50)[0]
    assert cut["truncated"] and len(cut["scores"]) == 50
    full = LR.merge_large_ref(table, boxes, scores, classes, counts, 1, 0.6, 0)[0]
    assert np.array_equal(cut["view_row"], full["view_row"][:50]) and np.array_equal(cut["view_index"], full["view_index"][:50])


def test_header_and_library_agree_on_the_large_merge():
    from sylph_amd import _lib
    text = open(os.path.join(ROOT, "include", "sylph_hip.h")).read()
    for ret, name, nargs in (("int64_t", "sylph_merge_views_large_bytes", 3), ("int", "sylph_merge_views_large", 24)):
        m = re.search(ret + r"\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"include/sylph_hip.h does not declare {name}"
        assert len(m.group(1).split(",")) == nargs
        assert len(_lib.PROTOTYPES[name][1]) == nargs
        assert hasattr(_lib.lib(), name)
    assert "MERGE_LARGE_POOL_CAP = 1048576" in text and "MERGE_POOL_CAP = 4096" in text
    assert V.MERGE_POOL_CAP == 4096


def test_workspace_size_function():
    from sylph_amd import _lib
    L = _lib.lib()
    small, big = L.sylph_merge_views_large_bytes(1, 1, 1), L.sylph_merge_views_large_bytes(3, 150, 100)
    assert 0 < small < big
    assert L.sylph_merge_views_large_bytes(1, 1 << 20, 1 << 11) == -1 and b"row index" in L.sylph_last_error()  # 2^31 rows
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        assert L.sylph_merge_views_large_bytes(*bad) == -1


def test_merge_route():
    assert V.merge_route([20], 200, None) == "block"
    assert V.merge_route([21], 200, None) == "large"
    assert V.merge_route([64], 64, None) == "block"  # exactly 4 096 rows
    assert V.merge_route([7, 20, 1], 200, None) == "block"
    assert V.merge_route([7, 21, 1], 200, None) == "large"
    assert V.merge_route([], 200, None) == "block"
    for topk in (0, 1, 100, 300):
        assert V.merge_route([1], 200, topk) == "large"


def test_a_twelve_megapixel_photo_needs_the_large_merge():
    vs = V.tile_views(3000, 4000, (800, 800), 0.2, 800, 1333)
    assert len(vs) > 20
    assert V.merge_route([len(vs)], 200, None) == "large"
