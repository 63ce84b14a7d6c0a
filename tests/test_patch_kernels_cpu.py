"""CPU side of tests/test_patch_kernels_gpu.py (no GPU, no library):
  * the restated patch geometry (tests/patch_ref.py) reproduces the values the C++ comments quote;
  * every case of the GPU tables is in the geometry class it is in the table for, and on the side of the conv_rw3 launch rule it
    claims -- a retune of pick_patch or of the rule that moves a case fails here by name;
  * the block bound of the GPU tests (2 bf16 ulps at max(|element|, rms)) catches a one-row and a one-column halo error at every
    identity-block shape of the tables: two wrong references, built from the oracle.bf16 pieces, break it."""
import pytest
import torch
import torch.nn.functional as F

import patch_ref as PR
from bf16_ulps import ulps
from test_patch_kernels_gpu import FUSED, RW3_BASIC, RW3_BOTTLENECK, STEM, _id, bottleneck_operands


def test_pick_patch_reproduces_the_documented_patches():
    """csrc/api_conv.hip pick_patch: the patches of the 800 x 1344 pyramid levels (and of the res2 map, csrc/conv_igemm.hip)"""
    want = {(100, 168): (10, 12), (50, 84): (10, 12), (25, 42): (9, 14), (13, 21): (13, 7), (7, 11): (7, 11), (200, 336): (8, 16)}
    assert {hw: PR.pick_patch(*hw) for hw in want} == want
    # "per image 188 patches of 128 = 24 064 positions for 22 400 real ones"
    assert sum(PR.geometry(1, h, w).tiles for h, w in list(want)[:5]) == 188
    assert sum(h * w for h, w in list(want)[:5]) == 22400


def test_picked_patches_fit_the_kernels_halo():
    """every patch pick_patch(H, W, 128, 184, 2) can return has at most 128 positions and a halo of at most 184 rows of the 192"""
    for H in range(1, 140, 7):
        for W in range(1, 140, 5):
            ph, pw = PR.pick_patch(H, W)
            assert ph * pw <= 128 and (ph + 2) * (pw + 2) <= 184 and 4 <= pw <= 32, (H, W, ph, pw)


def test_conv_rw3_patch_ok_is_pw_10_to_13_and_ph_up_to_10():
    for ph in range(1, 41):
        for pw in range(1, 41):
            assert PR.conv_rw3_patch_ok(ph, pw) == (10 <= pw <= 13 and ph <= 10 and ph * pw <= 128), (ph, pw)
    for pw in range(4, 15):  # the bank rule of rw_row_pitch: pitch / 16 == pw (mod 16), never below the natural pitch
        p = PR.rw_row_pitch(pw)
        assert p % 16 == 0 and (p // 16 - pw) % 16 == 0 and 0 <= p - (pw + 2) * PR.RW_TP < 256, (pw, p)


def test_conv_rw3_launch_rule():
    assert PR.RW3_MIN_POSITIONS == 30720
    assert PR.conv_rw3_route(2, 100, 168) == (10, 12) and PR.conv_rw3_route(1, 100, 168) is None  # "from 2 full-size images on"
    assert PR.conv_rw3_route(1, 100, 168, knob=2) == (10, 12) and PR.conv_rw3_route(64, 100, 168, knob=0) is None
    assert PR.conv_rw3_route(4, 93, 157) is None  # tests/test_bf16_pinned_gpu.py: "no conv_rw3 patch fits 93 x 157"
    assert PR.conv_rw3_route(500, 100, 168) is None and PR.conv_rw3_route(499, 100, 168) == (10, 12)  # 2 GiB buffer descriptors


# tiles of the launch and the rows / columns inside the last row / column of patches, as the GPU tables' comments state them
FUSED_GEOMETRY = {(1, 7, 7): (1, 7, 7), (3, 11, 13): (6, 11, 6), (2, 17, 23): (8, 8, 11), (3, 33, 47): (42, 16, 5), (1, 3, 130): (7, 3, 16),
                  (1, 130, 3): (8, 11, 3), (2, 2, 5): (2, 2, 5), (30, 26, 38): (270, 8, 12)}
RW3_GEOMETRY = {(64, 20, 24): (256, 10, 12), (63, 20, 24): (252, 10, 12), (79, 17, 23): (316, 8, 11), (25, 29, 43): (300, 9, 10),
                (11, 50, 58): (275, 10, 10), (16, 44, 44): (256, 11, 11), (32, 26, 38): (288, 8, 12)}


@pytest.mark.parametrize("case", FUSED, ids=[_id(c) for c in FUSED])
def test_fused_case_is_in_its_class(case):
    shape, patch, cls = case
    g = PR.geometry(*shape)
    assert (g.ph, g.pw) == patch, (shape, g)
    assert (g.tiles, g.last_rows, g.last_cols) == FUSED_GEOMETRY[shape], (shape, g)
    assert cls <= PR.classes(*shape), (shape, cls, PR.classes(*shape))


@pytest.mark.parametrize("case", RW3_BASIC + [RW3_BOTTLENECK], ids=[_id(c) for c in RW3_BASIC + [RW3_BOTTLENECK]])
def test_conv_rw3_case_is_in_its_class_and_on_its_side_of_the_launch_rule(case):
    shape, patch, cls = case
    B, H, W = shape
    g = PR.geometry(*shape)
    assert PR.conv_rw3_route(*shape) == patch, (shape, PR.conv_rw3_route(*shape))
    assert (g.tiles, g.last_rows, g.last_cols) == RW3_GEOMETRY[shape], (shape, g)
    assert cls <= PR.classes(*shape), (shape, cls, PR.classes(*shape))
    if patch is None:  # each off-case is off for ONE reason
        big, fits = B * H * W >= PR.RW3_MIN_POSITIONS, PR.conv_rw3_patch_ok(g.ph, g.pw)
        assert big != fits, (shape, big, fits)
    assert B * H * W * 256 < 1 << 31


def test_tables_reach_every_class_and_both_sides_of_the_rule():
    fused = set().union(*(PR.classes(*c[0]) for c in FUSED))
    assert fused == {"exact", "ragged_y", "ragged_x", "narrow", "few_tiles", "odd_walk", "second_patch"}, fused
    rw3 = [c for c in RW3_BASIC + [RW3_BOTTLENECK] if c[1]]
    assert set().union(*(PR.classes(*c[0]) for c in rw3)) >= {"exact", "ragged_y", "ragged_x", "odd_walk", "second_patch"}
    assert {c[1][1] for c in rw3} == {11, 12, 13}  # three of conv_rw3's four patch widths, i.e. three halo row pitches
    assert (64, 20, 24) in [c[0] for c in rw3] and 64 * 20 * 24 == PR.RW3_MIN_POSITIONS  # the rule's boundary itself
    off = [c[0] for c in RW3_BASIC if c[1] is None]
    assert any(B * H * W < PR.RW3_MIN_POSITIONS for B, H, W in off) and any(B * H * W >= PR.RW3_MIN_POSITIONS for B, H, W in off)
    # the stem's 8 x 16 output tiles: partial in both directions, and a map smaller than one tile
    outs = [((H - 1) // 2 + 1, (W - 1) // 2 + 1) for _, H, W in STEM]
    assert any(h % 8 and w % 16 and h > 8 and w > 16 for h, w in outs) and any(h < 8 and w < 16 for h, w in outs), outs


# ---- sensitivity: the block bound against a one-row / one-column halo error -------------------------------------------------------
def _identity_block_refs(x, ws, scales, shifts):
    """oracle.bf16.bottleneck of an identity block from its pieces -> (right, wrong_a, wrong_b):
      (a) conv1's output ring OUTSIDE the image left at relu(shift1) -- what conv1's epilogue makes of a zero halo input -- instead of
          being forced to 0 (conv2's padding): one row / column of outputs along each map edge sees it;
      (b) conv2 without the kw = 2 tap that reads the LAST COLUMN of the map (a halo one column short on the right: the outputs of
          column W - 2 lose that tap; at column W - 1 the tap reads the padding and dropping it would change nothing)."""
    from oracle import bf16 as OB16
    _, t1 = OB16.conv_epilogue(x, ws[0], scales[0], shifts[0], relu=True)
    w2 = OB16.r(ws[1])
    acc = F.conv2d(t1, w2, None, padding=1)

    def tail(acc2):
        t2 = OB16.r(F.relu(OB16.fma(acc2, scales[1].view(1, -1, 1, 1), shifts[1].view(1, -1, 1, 1))))
        return OB16.conv_epilogue(t2, ws[2], scales[2], shifts[2], relu=True, res_bf=x)[1]

    ring = OB16.r(F.relu(shifts[0])).view(1, -1, 1, 1)
    t1p = F.pad(t1, (1, 1, 1, 1))
    t1p[:, :, 0, :], t1p[:, :, -1, :], t1p[:, :, :, 0], t1p[:, :, :, -1] = ring[..., 0], ring[..., 0], ring[..., 0], ring[..., 0]
    acc_a = F.conv2d(t1p, w2, None)
    W = x.shape[3]
    acc_b = acc.clone()
    acc_b[:, :, :, W - 2:W - 1] -= F.conv2d(t1[:, :, :, W - 1:W], w2[:, :, :, 2:3], None, padding=(1, 0))
    return tail(acc), tail(acc_a), tail(acc_b)


SENSITIVITY = [(c[0], 256, 64, 256) for c in FUSED] + [(RW3_BOTTLENECK[0], 512, 128, 512)]


@pytest.mark.parametrize("case", SENSITIVITY, ids=[f"{_id(c[0])}_C{c[1]}" for c in SENSITIVITY])
def test_block_bound_catches_a_one_row_or_one_column_halo_error(case):
    from oracle import bf16 as OB16
    shape, cin, mid, cout = case
    x, ws, scales, shifts = bottleneck_operands(shape, cin, mid, cout, False)
    right, wrong_a, wrong_b = _identity_block_refs(x, ws, scales, shifts)
    assert torch.equal(right, OB16.bottleneck(x, ws, scales, shifts, 1)), "the pieces do not restate oracle.bf16.bottleneck"
    assert int((shifts[0] > 0).sum()) >= mid // 4  # (a) needs channels whose ring value relu(shift1) is not 0
    for name, wrong in (("ring left at relu(shift1)", wrong_a), ("kw = 2 tap of the last column dropped", wrong_b)):
        frac, worst = ulps(wrong, right, "rms")
        print(f"{_id(shape)} {name}: {frac * 100:.2f} % of elements differ, worst {worst:.1f} bf16 ulp")
        assert worst > 2.0, f"{_id(shape)}: the block bound would not notice '{name}' ({worst:.2f} ulp)"
