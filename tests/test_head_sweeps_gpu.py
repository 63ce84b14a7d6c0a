"""The head's persistent streaming kernels where a wave takes SEVERAL row groups.

gn_logits_kernel<false>, gn_logits_kernel<true> (episodes), gn_taps_kernel<2> (csrc/head_fused.hip) and logits_scan_kernel
(csrc/detect.hip) launch min(n_tiles, CAP) blocks over the head's 128-row tile table.  Up to CAP tiles (11 full-size images) every wave
runs its loop body once; above, it goes round again and carries state from one row group to the next: the wave-private GroupNorm
coefficient table (reloaded on a segment change only), in logits_scan_kernel the code fragments and biases of the NEXT class tile (the
last tile of a group reloads tile 0) and the wave's candidate list (flushed to the counter of the segment it leaves), in the episodes
form the code block (reloaded when the next tile's image belongs to another episode).  Every benchmark batch runs there; the tests that
compare these kernels with a reference elsewhere stop below the cap.

The regime needs many TILES, not many rows: the table has at least one tile per (image, level), so a few hundred tiny pyramids cross
the cap.  Two geometries (padded size -> level maps -> tiles per image):
  (96, 160): 12x20, 6x10, 3x5, 2x3, 1x2  -> 2 + 1 + 1 + 1 + 1 = 6 tiles, 323 rows.  Level 0 ends in a 16-row group, level 1 in a 28-row
             group, three levels are smaller than one 32-row group (waves 1-3 of their block skip them and keep their state).
             CAP mod 6 = 2: the tiles a block takes one grid stride apart lie on other levels of other images.
             B = 704: 4224 tiles, three sweeps (blocks 0-127), B = 352: 2112 tiles, two (blocks 0-63).
  (64, 112): 8x14, 4x7, 2x4, 1x2, 1x1    -> 5 tiles (one per level), 151 rows; B = 832: 4160 tiles, an episodes block takes a run of
             ceil(4160 / CAP) = 3 tiles, which straddles images (6 tiles per image would put every run inside one image).
All images are distinct (random bf16-rounded features through Engine.import_pyramid: no backbone runs).  Every case asserts its premises
from the level shapes -- tile count, sweeps, other segment and level one grid stride on -- and, from the profile, the kernel that ran.

References and bounds (none of them new):
  * logits / box / ctrness / iou of EVERY image and level against oracle.bf16 on the operands the HIP graph itself stored (the last
    tower layers' outputs and coefficient tables): the project's bound for fp32 head outputs, 1e-4 of the output scale (_assert_f32);
  * the episodes form also bit for bit (torch.equal) against the uniform head of each episode's codes;
  * logits_scan_kernel: every field of every image torch.equal with a decode of the exported (unfused) logits, and the oracle's
    decode of those exported outputs on the first and last image of every sweep.  The decode is made transparent -- NMS threshold 1
    (nothing is suppressed), post-NMS cut and output rows at 5 levels x PRE_NMS_TOPK -- so that the comparison sees the candidates and
    not only the survivors: segments with fewer than PRE_NMS_TOPK candidates show their whole candidate set, level-0 segments with more
    exercise the select; both kinds are counted on the exported logits and asserted.
A failure names image, level and the sweep (or run position) of the tile."""
import numpy as np
import pytest
import torch

from test_bf16_pinned_gpu import _assert_f32
from test_hip_parity import _cfg
from test_mixed_episodes_gpu import FIELDS, _code, _kernels, _pairs

pytestmark = pytest.mark.gpu

CAP = 2048  # HEAD_STREAM_MAX_BLOCKS (csrc/kernels.h): blocks of one launch of the four kernels
HW, LEVELS = (96, 160), [(12, 20), (6, 10), (3, 5), (2, 3), (1, 2)]
HW_EP, LEVELS_EP = (64, 112), [(8, 14), (4, 7), (2, 4), (1, 2), (1, 1)]
TOPK = 100             # PRE_NMS_TOPK_TEST of the scan cases
MAX_OUT = 5 * TOPK + 12


def _tile_table(B, levels):
    """(image, level, first row) of every 128-row tile in the order of the head's tile table (image-major, level, row)"""
    return [(b, l, r) for b in range(B) for l, (h, w) in enumerate(levels) for r in range(0, h * w, 128)]


def _premises(eng, B, hw, levels, n_tiles, sweeps):
    """(a) tile count and sweeps as the case states them, (b) one grid stride on: another image and another level, (c) a ragged last
    group and a level smaller than one group -> the tile table"""
    assert eng.level_shapes(*hw) == levels
    tiles = _tile_table(B, levels)
    assert len(tiles) == B * sum(-(-h * w // 128) for h, w in levels) == n_tiles
    assert -(-n_tiles // CAP) == sweeps and sweeps >= 2, (n_tiles, sweeps)
    for t in range(n_tiles - CAP):
        (b0, l0, _), (b1, l1, _) = tiles[t], tiles[t + CAP]
        assert b0 != b1 and l0 != l1, f"tiles {t} and {t + CAP} share an image or a level"
    assert any(h * w > 32 and (h * w) % 32 for h, w in levels) and any(h * w < 32 for h, w in levels)
    return tiles


def _tile_of(levels, i, l, row):
    per_image = [-(-h * w // 128) for h, w in levels]
    return i * sum(per_image) + sum(per_image[:l]) + row // 128


def _where_sweep(levels):
    return lambda i, l, row: f"tile {_tile_of(levels, i, l, row)}, sweep {_tile_of(levels, i, l, row) // CAP} of its block"


def _pin(got, want, what, level, where, images=None):
    """_assert_f32 (1e-4 of the output scale); a failure names the worst element's image, level, row and sweep"""
    try:
        _assert_f32(got, want, what)
    except AssertionError as e:
        d = (got.float().cpu() - want.float().cpu()).abs().flatten(2).amax(1)  # (images, rows)
        j = int(d.amax(1).argmax())
        row = int(d[j].argmax())
        i = images[j] if images is not None else j
        raise AssertionError(f"{e}; worst at image {i}, level {level}, row {row}: {where(i, level, row)}") from None


def _pyramid(B, levels, seed):
    """B images of random bf16-representable features, (d) all distinct: their per-image sums differ on every level"""
    from oracle import bf16 as OB16
    g = torch.Generator().manual_seed(seed)
    feats = [OB16.r(torch.randn(B, 256, h, w, generator=g)) for h, w in levels]
    for f in feats:
        assert len(set(f.double().sum((1, 2, 3)).tolist())) == B, "two images of the batch are equal"
    return feats


@pytest.fixture(scope="module")
def pyr():
    return _pyramid(704, LEVELS, seed=11)


@pytest.fixture(scope="module")
def sd():
    from sylph_amd import synthetic as Wt
    return Wt.head_state_dict(seed=1, num_classes=60)


def _new(cfg, sd, feats, hw, **kw):
    from sylph_amd.engine import Engine
    eng = Engine(cfg, dtype="bf16", **kw)
    eng.load_state_dict(sd)
    eng.set_debug_taps(True)
    eng.import_pyramid(feats, hw)
    return eng


def _normalised(eng, tower):
    """relu(GroupNorm(.)) of the last layer of a tower as its consumers feed it to their MFMAs, per level on the host: oracle.bf16.gn_apply
    of the stored conv output and the coefficient table the HIP graph left"""
    from oracle import bf16 as OB16
    ys, cfs = eng.export_tower(tower, 3)
    return [OB16.gn_apply(y.cpu(), cf.cpu()) for y, cf in zip(ys, cfs)]


# ------------------------------------------------------------------------------------------------ A: gn_logits<false>, gn_taps: three sweeps
@pytest.fixture(scope="module")
def three_sweeps(pyr, sd):
    """One engine over the 704-image batch; the normalised last tower layers (they do not depend on the class codes) computed once"""
    eng = _new(_cfg(), sd, pyr, HW)
    _premises(eng, 704, HW, LEVELS, n_tiles=4224, sweeps=3)
    c = _code("n5")
    k = _kernels(eng, lambda: eng.head(c["cls_conv"], c["cls_bias"]))
    case = {"eng": eng, "kernels": k, "cls": _normalised(eng, 0), "box": _normalised(eng, 1)}
    yield case
    eng.close()


@pytest.mark.parametrize("name", ["n5", "n32"])
def test_gn_logits_three_sweeps(three_sweeps, name):
    """gn_logits_kernel<false> at 4224 tiles: every block takes a second tile, blocks 0-127 a third.  n5: the narrow 8-float logits
    pitch, n32: the full class tile."""
    from oracle import bf16 as OB16
    eng, c = three_sweeps["eng"], _code(name)
    k = _kernels(eng, lambda: eng.head(c["cls_conv"], c["cls_bias"]))
    assert k.get("gn_logits_kernel") == 1 and "logits_scan_kernel" not in k and "gn_logits_episodes_kernel" not in k, k
    lo = eng.export_head()[0]
    for l in range(5):
        assert lo[l].shape[1] == c["cls_conv"].shape[0]
        want = OB16.cls_logits(three_sweeps["cls"][l], c["cls_conv"].cpu(), c["cls_bias"].cpu())
        _pin(lo[l], want, f"{name} logits level {l}", l, _where_sweep(LEVELS))


def test_gn_taps_three_sweeps(three_sweeps, sd):
    """gn_taps_kernel<2> + tap_gather_kernel on the same table: box regression, centerness and IoU of every image and level"""
    from oracle import bf16 as OB16
    eng, c = three_sweeps["eng"], _code("n5")
    k = _kernels(eng, lambda: eng.head(c["cls_conv"], c["cls_bias"]))
    assert k.get("gn_taps_kernel+tap_gather_kernel") == 1 and three_sweeps["kernels"].get("gn_taps_kernel+tap_gather_kernel") == 1, k
    _, rg, ct, io = eng.export_head()
    for l in range(5):
        reg, ctr, iou = OB16.predictions(three_sweeps["box"][l], sd, l)
        for got, want, what in ((rg, reg, "reg"), (ct, ctr, "ctrness"), (io, iou, "iou")):
            _pin(got[l], want, f"{what} level {l}", l, _where_sweep(LEVELS))


# ------------------------------------------------------------------------------------------------ B: gn_logits<true>: runs of three tiles
def test_gn_logits_episodes_runs_of_three_tiles(sd):
    """gn_logits_kernel<true> at 4160 tiles: block b takes tiles 3b, 3b + 1, 3b + 2.  Episodes of 1, 5, 20 and 32 classes, two images
    each in turn: the episode changes inside some runs (the code block is reloaded mid-run), other runs hold two images of one episode
    (the segment changes, the code block stays), and neighbouring runs continue an episode."""
    from oracle import bf16 as OB16
    B, n_tiles = 832, 4160
    feats = _pyramid(B, LEVELS_EP, seed=12)
    eng = _new(_cfg(), sd, feats, HW_EP)
    tiles = _premises(eng, B, HW_EP, LEVELS_EP, n_tiles=n_tiles, sweeps=3)
    run = -(-n_tiles // CAP)
    assert run == 3
    ie = [(i // 2) % 4 for i in range(B)]
    runs = [tiles[t:t + run] for t in range(0, n_tiles, run)]
    n_change = sum(len({ie[b] for b, _, _ in r}) > 1 for r in runs)
    n_keep = sum(len({b for b, _, _ in r}) > 1 and len({ie[b] for b, _, _ in r}) == 1 for r in runs)
    n_cont = sum(ie[a[-1][0]] == ie[b[0][0]] for a, b in zip(runs, runs[1:]))
    print(f"{len(runs)} runs of {run} tiles: the episode changes inside {n_change}, {n_keep} hold two images of one episode, "
          f"{n_cont} continue their predecessor's episode")
    assert n_change > 100 and n_keep > 100 and n_cont > 100
    for r in runs:  # consecutive tiles of a run: other segments, other levels
        assert all((a[0], a[1]) != (b[0], b[1]) and a[1] != b[1] for a, b in zip(r, r[1:]))
    names = ("n1", "n5", "n20", "n32")
    codes = [_code(n) for n in names]
    k = _kernels(eng, lambda: eng.head_episodes(_pairs(codes), ie))
    assert k.get("gn_logits_episodes_kernel") == 1 and "gn_logits_kernel" not in k and "logits_scan_kernel" not in k, k
    lo = eng.export_head()[0]
    xn = _normalised(eng, 0)
    where = lambda i, l, row: f"tile {_tile_of(LEVELS_EP, i, l, row)}, position {_tile_of(LEVELS_EP, i, l, row) % run} of its run"
    mine = [[i for i in range(B) if ie[i] == e] for e in range(4)]
    for e, c in enumerate(codes):
        n = c["cls_conv"].shape[0]
        for l in range(5):
            assert lo[l].shape[1] == 32
            want = OB16.cls_logits(xn[l][mine[e]], c["cls_conv"].cpu(), c["cls_bias"].cpu())
            _pin(lo[l][mine[e], :n], want, f"episode {names[e]} logits level {l}", l, where, images=mine[e])
    for e, c in enumerate(codes):  # ... and bit for bit what the uniform head of the episode's codes gives these images
        n = c["cls_conv"].shape[0]
        eng.head(c["cls_conv"], c["cls_bias"])
        uni = eng.export_head()[0]
        for l in range(5):
            a, b = lo[l][mine[e], :n], uni[l][mine[e]]
            if not torch.equal(a, b):
                j = int((a != b).flatten(1).any(1).nonzero()[0])
                row = int((a[j] != b[j]).any(0).flatten().nonzero()[0])
                raise AssertionError(f"episode {names[e]}: logits of image {mine[e][j]}, level {l}, row {row} differ from the uniform head's: "
                                     f"{where(mine[e][j], l, row)}")
    eng.close()


# ------------------------------------------------------------------------------------------------ C: logits_scan_kernel: two and three sweeps
def _transparent_cfg(thr, bq=("ctrness",), twc=False):
    return _cfg(**{"MODEL.FCOS.INFERENCE_TH_TEST": thr, "MODEL.FCOS.PRE_NMS_TOPK_TEST": TOPK, "MODEL.FCOS.NMS_TH": 1.0,
                   "MODEL.FCOS.POST_NMS_TOPK_TEST": 5 * TOPK, "MODEL.FCOS.BOX_QUALITY": list(bq), "MODEL.FCOS.THRESH_WITH_CTR": twc})


def _candidate_counts(lo, ct, io, thr, bq, twc):
    """(B, 5) candidates per (image, level) of exported head outputs, the reference's test (oracle.decode.decode_level)"""
    out = []
    for l in range(5):
        p = lo[l].sigmoid()
        if twc:
            c, q = ct[l].sigmoid(), io[l].sigmoid()
            p = p * {("ctrness",): c, ("iou",): q, ("ctrness", "iou"): torch.sqrt(q * c)}[tuple(sorted(bq))]
        out.append((p > thr).flatten(1).sum(1))
    return torch.stack(out, 1).cpu()


def _sweep_images(B, levels):
    """first and last image with a tile in each sweep of the table, and the sweeps each of them has tiles in"""
    sweeps = {}
    for t, (b, _, _) in enumerate(_tile_table(B, levels)):
        sweeps.setdefault(t // CAP, []).append(b)
    pick = sorted({v for bs in sweeps.values() for v in (bs[0], bs[-1])})
    return pick, {i: sorted(s for s, bs in sweeps.items() if i in bs) for i in pick}, len(sweeps)


def _same_detections(got, want, what):
    assert got["scores"].numel() == want["scores"].numel(), f"{what}: {got['scores'].numel()} detections, expected {want['scores'].numel()}"
    for f in FIELDS:
        assert torch.equal(got[f], want[f]), f"{what}: {f} differs"


SCAN_CASES = [
    # id, batch, tiles, sweeps, classes, code scale, threshold, BOX_QUALITY, THRESH_WITH_CTR
    ("866way_two_sweeps", 352, 2112, 2, 866, 1.5, 0.1, ("ctrness",), False),   # 28 class tiles, the last one partial, one wrap per wave
    ("40way_three_sweeps", 704, 4224, 3, 40, 3.0, 0.05, ("ctrness",), False),  # two class tiles, 24 of the second's 32 biases are -inf
    ("866way_two_sweeps_thresh_with_ctr", 352, 2112, 2, 866, 1.5, 0.05, ("ctrness", "iou"), True),
]


@pytest.mark.parametrize("case", SCAN_CASES, ids=[c[0] for c in SCAN_CASES])
def test_logits_scan_sweeps(pyr, sd, case):
    from oracle import decode as OD
    from sylph_amd import synthetic as Wt
    _, B, n_tiles, sweeps, N, scale, thr, bq, twc = case
    feats = [f[:B] for f in pyr]
    cfg = _transparent_cfg(thr, bq, twc)
    codes = Wt.synthetic_codes(N, seed=77, scale=scale)
    # the unfused logits first, from an engine that is never decoded (its scan's candidates are not read): the candidate capacity of the
    # engine under test is sized from them, 2 x the fullest segment, instead of the default that holds every score of level 0
    ref = _new(cfg, sd, feats, HW, cand_cap=4096)
    ref.head(codes["cls_conv"], codes["cls_bias"])
    ref_lo, _, ref_ct, ref_io = ref.export_head()
    cnt = _candidate_counts(ref_lo, ref_ct, ref_io, thr, bq, twc)
    ref.close()
    n_few = int(((cnt > 0) & (cnt < TOPK)).sum())
    n_many0 = int((cnt[:, 0] > TOPK).sum())
    cap = (2 * int(cnt.max()) + 1023) // 1024 * 1024
    print(f"{case[0]}: candidates per (image, level): min {cnt.min(0).values.tolist()}, max {cnt.max(0).values.tolist()}; {n_few} of {cnt.numel()} "
          f"segments hold 1 .. {TOPK - 1} candidates, {n_many0} of {B} level-0 segments more than {TOPK}; cand_cap {cap}")
    assert n_few >= B and n_many0 >= B // 2, (n_few, n_many0)

    eng = _new(cfg, sd, feats, HW, cand_cap=cap)
    _premises(eng, B, HW, LEVELS, n_tiles=n_tiles, sweeps=sweeps)
    k = _kernels(eng, lambda: eng.head(codes["cls_conv"], codes["cls_bias"]))
    assert k.get("logits_scan_kernel") == 1 and "gn_logits_kernel" not in k and k.get("gn_taps_kernel+tap_gather_kernel") == 1, k
    fused = eng.decode(max_out=MAX_OUT)
    lo, rg, ct, io = eng.export_head()  # runs the unfused conv on the same tower output
    for l in range(5):
        assert torch.equal(lo[l], ref_lo[l]), f"level {l}: the two engines' exported logits differ (the counts above are not this run's)"
    eng.import_head(lo, rg, ct, io)     # ... and its logits go through decode_scan_kernel
    unfused = eng.decode(max_out=MAX_OUT)
    per_image = sum(-(-h * w // 128) for h, w in LEVELS)
    for i in range(B):
        t0 = i * per_image
        _same_detections(fused[i], unfused[i], f"image {i} (tiles {t0} .. {t0 + per_image - 1}, sweeps {t0 // CAP} .. {(t0 + per_image - 1) // CAP}): "
                                               "fused scan vs decode of the exported logits")
    # the oracle's decode on the first and last image of every sweep
    pick, in_sweeps, n_sweeps = _sweep_images(B, LEVELS)
    assert n_sweeps == sweeps and all(any(s in in_sweeps[i] for i in pick) for s in range(sweeps)), in_sweeps
    heads = [[t[pick].cpu() for t in ts] for ts in (lo, rg, ct, io)]
    want = OD.predict_proposals(*heads, pre_nms_thresh=thr, pre_nms_topk=TOPK, nms_thresh=1.0, post_nms_topk=5 * TOPK,
                                thresh_with_ctr=twc, box_quality=bq)
    cnt_pick = _candidate_counts(heads[0], heads[2], heads[3], thr, bq, twc)
    for j, i in enumerate(pick):
        what = f"image {i} (sweeps {in_sweeps[i]}) vs the oracle's decode"
        # nothing suppressed, nothing cut after the per-level top-k: the oracle keeps every level's candidates, at most TOPK each
        assert want[j]["scores"].numel() == int(cnt_pick[j].clamp(max=TOPK).sum()), what
        w, g = OD.detector_postprocess(want[j], HW, HW[0], HW[1]), fused[i]
        assert w["scores"].numel() > TOPK, what
        assert g["scores"].numel() == w["scores"].numel(), f"{what}: {g['scores'].numel()} detections, expected {w['scores'].numel()}"
        np.testing.assert_array_equal(g["fpn_levels"].cpu().numpy(), w["fpn_levels"].numpy(), err_msg=what)
        np.testing.assert_array_equal(g["pred_classes"].cpu().numpy(), w["pred_classes"].numpy(), err_msg=what)
        np.testing.assert_array_equal(g["locations"].cpu().numpy(), w["locations"].numpy(), err_msg=what)
        np.testing.assert_allclose(g["scores"].cpu().numpy(), w["scores"].numpy(), atol=1e-5, err_msg=what)
        np.testing.assert_allclose(g["pred_boxes"].cpu().numpy(), w["pred_boxes"].numpy(), atol=1e-3, err_msg=what)
    eng.close()


# ------------------------------------------------------------------------------------------------ D: a many-way episode's tile sub-list
def test_many_way_episode_sublist_two_sweeps_next_to_few_way(pyr, sd):
    """The per-episode launches of a mixed head: logits_scan_kernel over the tile sub-list of a 60-way episode that owns 352 of 396
    images -- 2112 tiles, two sweeps -- next to a 5-way and a 20-way episode (every ninth image, in turn).  Every image gets, bit for
    bit, what the uniform head of its episode's codes gives it on the same batch (there the scan walks all 2376 tiles: the same row
    groups, taken by other waves in other company)."""
    B = 396
    ie = [(1 + (i // 9) % 2) if i % 9 == 8 else 0 for i in range(B)]
    per_image = sum(-(-h * w // 128) for h, w in LEVELS)
    many = [i for i in range(B) if ie[i] == 0]
    assert len(many) * per_image == 2112 > CAP and -(-2112 // CAP) == 2
    sub = [t for t in _tile_table(B, LEVELS) if ie[t[0]] == 0]  # the episode's sub-list, in table order
    assert len(sub) == 2112 and all(a[0] != b[0] and a[1] != b[1] for a, b in zip(sub, sub[CAP:]))
    codes = [_code("n60"), _code("n5"), _code("n20")]
    eng = _new(_transparent_cfg(0.05), sd, [f[:B] for f in pyr], HW)
    assert eng.level_shapes(*HW) == LEVELS
    want = [None] * B
    for e, c in enumerate(codes):
        k = _kernels(eng, lambda: eng.head(c["cls_conv"], c["cls_bias"]))
        assert (k.get("logits_scan_kernel") == 1) == (e == 0) and (k.get("gn_logits_kernel") == 1) == (e != 0), k
        d = eng.decode(max_out=MAX_OUT)
        for i in range(B):
            if ie[i] == e:
                assert d[i]["scores"].numel() > 0, f"uniform run of episode {e}: image {i} has no detection -- the comparison proves nothing"
                want[i] = d[i]
    k = _kernels(eng, lambda: eng.head_episodes(_pairs(codes), ie))
    assert k.get("logits_scan_kernel") == 1 and k.get("gn_logits_kernel") == 2 and "gn_logits_episodes_kernel" not in k, k
    got = eng.decode(max_out=MAX_OUT)
    for i in range(B):
        pos = many.index(i) * per_image if ie[i] == 0 else None
        _same_detections(got[i], want[i], f"image {i} (episode {ie[i]}" + (f", sub-list tiles {pos} .. {pos + per_image - 1}, sweeps "
                         f"{pos // CAP} .. {(pos + per_image - 1) // CAP}" if pos is not None else "") + ") vs the uniform head")
    eng.close()
