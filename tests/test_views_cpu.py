"""Query views, host side (no GPU): the planners of sylph_amd.views, the merge reference of tests/views_ref.py against a brute-force
restatement and against the oracle's NMS, the TEST.AUG config keys, and the C ABI's declarations."""
import os
import re

import numpy as np
import pytest

import views_ref as VR
from sylph_amd import views as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- planners --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(480, 640), (1200, 1600), (1000, 400), (37, 53)])
def test_tta_views_follow_resize_shortest_edge(h, w):
    from sylph_amd.predictor import resize_shortest_edge_shape
    sizes, max_size = (400, 600, 800, 1200), 1333
    for flip in (False, True):
        vs = V.tta_views(h, w, sizes, max_size, flip)
        assert len(vs) == len(sizes) * (2 if flip else 1)
        per = 2 if flip else 1
        for k, s in enumerate(sizes):
            for j in range(per):
                v = vs[k * per + j]
                assert v["crop"] == (0, 0, w, h)
                assert v["size"] == resize_shortest_edge_shape(h, w, s, max_size)
                assert v["flip"] == (j == 1)  # DatasetMapperTTA: the mirrored twin right behind the plain view


@pytest.mark.parametrize("h,w,tile,overlap", [(150, 200, (96, 96), 0.25), (3000, 4000, (1667, 1539), 0.2), (100, 100, (100, 100), 0.5),
                                               (97, 301, (64, 50), 0.0), (50, 70, (96, 96), 0.3)])
def test_tiles_cover_every_pixel_and_stay_inside(h, w, tile, overlap):
    vs = V.tile_views(h, w, tile, overlap, None, 4000, full_frame=False)
    th, tw = min(tile[0], h), min(tile[1], w)
    cover = np.zeros((h, w), dtype=bool)
    for v in vs:
        x0, y0, cw, ch = v["crop"]
        assert (cw, ch) == (tw, th), "every tile has the full tile size"
        assert x0 >= 0 and y0 >= 0 and x0 + cw <= w and y0 + ch <= h
        assert v["size"] == (th, tw) and not v["flip"]
        cover[y0:y0 + ch, x0:x0 + cw] = True
    assert cover.all()
    assert len({v["crop"] for v in vs}) == len(vs), "no tile twice"
    full = V.tile_views(h, w, tile, overlap, 96, 160)
    assert full[0]["crop"] == (0, 0, w, h) and full[0]["size"] == V.resize_shortest_edge_shape(h, w, 96, 160)
    assert [v["crop"] for v in full[1:]] == [v["crop"] for v in vs]
    assert all(v["size"] == V.resize_shortest_edge_shape(th, tw, 96, 160) for v in full[1:])


def test_tile_grid_of_the_benchmark():
    vs = V.tile_views(3000, 4000, (1667, 1539), 0.2, 800, 1333)
    assert len(vs) == 7  # the full frame + 2 x 3 tiles
    assert sorted({v["crop"][1] for v in vs[1:]}) == [0, 3000 - 1667] and sorted({v["crop"][0] for v in vs[1:]}) == [0, 1231, 4000 - 1539]


def test_plan_view_steps():
    views = []
    for h, w in [(96, 128), (120, 90), (1200, 1600), (480, 640)] * 5:
        views += V.tta_views(h, w, (64, 96, 400), 1333, True)
    for mb in (1, 4, 7, 192):
        steps = V.plan_view_steps(views, mb)
        assert steps == V.plan_view_steps(list(views), mb), "deterministic"
        flat = [i for st in steps for i in st]
        assert sorted(flat) == list(range(len(views))), "every view once"
        for st in steps:
            assert 1 <= len(st) <= mb
            assert st == sorted(st)
            pads = {((views[i]["size"][0] + 31) // 32, (views[i]["size"][1] + 31) // 32) for i in st}
            assert len(pads) == 1, "a step's views share their padded size: a small view is not padded to a large batch"
    assert max(len(st) for st in V.plan_view_steps(views * 40)) <= 192  # the default
    with pytest.raises(ValueError):
        V.plan_view_steps(views, 0)


def test_check_views_refuses_by_name():
    ok = [V.make_view((5, 7, 29, 31), (44, 40))]
    assert V.check_views(ok, 64, 48) == ok
    with pytest.raises(ValueError, match="leaves its"):
        V.check_views([V.make_view((30, 0, 29, 10), (10, 10))], 64, 48)
    with pytest.raises(ValueError, match="positive"):
        V.check_views([V.make_view((0, 0, 0, 10), (10, 10))], 64, 48)
    with pytest.raises(ValueError, match="empty"):
        V.check_views([], 64, 48)


# ---- the merge reference -----------------------------------------------------------------------------------------------------------
def interleaved_table():
    """3 sources with 1, 4 and 7 views, interleaved; flips and non-zero offsets"""
    order = [1, 2, 0, 2, 1, 2, 2, 1, 2, 2, 1, 2]
    rng = np.random.RandomState(3)
    table = []
    for k, s in enumerate(order):
        x0, y0 = (0, 0) if k % 4 == 0 else (int(rng.randint(0, 60)), int(rng.randint(0, 40)))
        table.append({"source": s, "crop": (x0, y0, 260 - x0, 200 - y0), "flip": k % 3 == 1})
    return table


MERGE_COUNTS = [16, 0, 9, 16, 5, 16, 1, 16, 12, 0, 16, 7]


@pytest.fixture(scope="module")
def merge_case():
    table = interleaved_table()
    boxes, scores, classes, counts = VR.draw_rows(table, 16, MERGE_COUNTS, 3, seed=11, thr=0.6, score_levels=12)
    return table, boxes, scores, classes, counts


@pytest.mark.parametrize("thr,K", [(0.6, 100), (0.6, 5), (0.3, 0), (0.0, 7), (0.0, 0)])
def test_merge_ref_against_bruteforce(merge_case, thr, K):
    table, boxes, scores, classes, counts = merge_case
    assert VR.min_iou_margin(table, boxes, scores, classes, counts, 3, thr) >= (1e-4 if thr == 0.6 else 0)
    a = VR.merge_ref(table, boxes, scores, classes, counts, 3, thr, K)
    b = VR.merge_bruteforce(table, boxes, scores, classes, counts, 3, thr, K)
    for s in range(3):
        for key in ("pred_boxes", "scores", "pred_classes", "view_index", "view_row"):
            assert np.array_equal(a[s][key], b[s][key]), (s, key)
    if thr == 0.0 and K == 0:  # everything, in stable score order
        for s in range(3):
            n = sum(c for c, t in zip(MERGE_COUNTS, table) if t["source"] == s)
            assert len(a[s]["scores"]) == n and np.all(np.diff(a[s]["scores"]) <= 0)
            same = np.diff(a[s]["scores"]) == 0
            key = a[s]["view_index"] * 16 + a[s]["view_row"]
            assert np.all(np.diff(key)[same] > 0), "ties: lower view first, then lower row"


def test_merge_ref_against_oracle_nms(merge_case):
    """ml_nms + the post-NMS keep of the oracle (oracle/decode.py) on the transformed union"""
    import torch
    from oracle import decode as OD
    table, boxes, scores, classes, counts = merge_case
    for K in (100, 5):
        got = VR.merge_ref(table, boxes, scores, classes, counts, 3, 0.6, K)
        for s in range(3):
            pool = [(v, r) for v in range(len(table)) if table[v]["source"] == s for r in range(int(counts[v]))]
            pb = np.array([VR.to_source(boxes[v, r], table[v]) for v, r in pool], dtype=np.float32).reshape(-1, 4)
            inst = {"pred_boxes": torch.from_numpy(pb), "scores": torch.tensor([float(scores[v, r]) for v, r in pool]),
                    "pred_classes": torch.tensor([int(classes[v, r]) for v, r in pool], dtype=torch.int64)}
            want = OD.select_over_all_levels(inst, 0.6, K)
            assert np.array_equal(got[s]["pred_boxes"], want["pred_boxes"].numpy())
            assert np.array_equal(got[s]["scores"], want["scores"].numpy())
            assert np.array_equal(got[s]["pred_classes"], want["pred_classes"].numpy())


def test_kth_place_tie_is_kept(merge_case):
    table, boxes, scores, classes, counts = merge_case
    full = VR.merge_ref(table, boxes, scores, classes, counts, 3, 0.6, 0)[2]["scores"]
    ties = [k for k in range(1, len(full)) if full[k] == full[k - 1]]
    assert ties, "the quantised scores give the kept list a tie"
    K = ties[0]  # the K-th and the (K+1)-th kept box share a score
    cut = VR.merge_ref(table, boxes, scores, classes, counts, 3, 0.6, K)[2]["scores"]
    assert len(cut) > K and np.all(cut[K:] == cut[K - 1])


# ---- config, C ABI ------------------------------------------------------------------------------------------------------------------
def test_test_aug_keys_load(tmp_path):
    from sylph_amd.config import get_default_cfg
    cfg = get_default_cfg()
    assert cfg.TEST.AUG.ENABLED is False and cfg.TEST.AUG.FLIP is True and int(cfg.TEST.AUG.MAX_SIZE) == 4000
    assert tuple(cfg.TEST.AUG.MIN_SIZES) == (400, 500, 600, 700, 800, 900, 1000, 1100, 1200)
    y = tmp_path / "tta.yaml"
    y.write_text("TEST:\n  AUG:\n    ENABLED: True\n    MIN_SIZES: (400, 800)\n    MAX_SIZE: 1333\n    FLIP: False\n")
    cfg.merge_from_file(str(y))
    assert cfg.TEST.AUG.ENABLED is True and tuple(cfg.TEST.AUG.MIN_SIZES) == (400, 800) and cfg.TEST.AUG.MAX_SIZE == 1333
    assert cfg.TEST.AUG.FLIP is False and int(cfg.TEST.REPEAT_TEST) == 1


def test_header_and_library_agree_on_the_view_symbols():
    from sylph_amd import _lib
    text = open(os.path.join(ROOT, "include", "sylph_hip.h")).read()
    for name, nargs in (("sylph_preprocess_views", 15), ("sylph_merge_views", 21)):
        m = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"include/sylph_hip.h does not declare {name}"
        assert len(m.group(1).split(",")) == nargs
        assert len(_lib.PROTOTYPES[name][1]) == nargs
        assert hasattr(_lib.lib(), name)
    assert "MERGE_POOL_CAP = 4096" in text
