"""LDS swizzle proof of conv_hpipe_kernel's 16x16x32 fragment reads (csrc/conv_hpipe.hip, "LDS images"), on the CPU.

The kernel reads its MFMA operands with ds_read_b128: lane l takes row l & 15 of a 16-row operand block and 16-byte k chunk
l >> 4.  A ds_read_b128 is serviced in four groups of 16 lanes, and within a group every lane must hit a different 16-byte
bank unit ((byte address >> 4) mod 16) or the read takes extra LDS cycles.  This file restates the kernel's address arithmetic
for the weight stage and the input halo, enumerates every lane group of every fragment read -- each tap of the 3x3 filter,
each patch shape the host can pick, both wave rows, all pad positions -- and checks that
  * the 16 lanes of a group hit 16 distinct bank units, and
  * the slot a lane reads holds the chunk it asks for (the re-pack / the halo load put it there with the same XOR).
"""
import itertools

import pytest

# ds_read_b128 lane groups (one LDS cycle each when conflict-free)
GROUPS = [[*range(0, 4), *range(12, 16), *range(20, 28)], [*range(4, 12), *range(16, 20), *range(28, 32)]]
GROUPS += [[l + 32 for l in g] for g in GROUPS]

BSTAGE = 256 * 64
HPROWS = 256
HALO_OFF = 4 * BSTAGE
HBUF = 2 * HPROWS * 64
XPAD = 4  # halo row pitch pw + 4 (api_conv.hip make_geom_patch for conv_hpipe)


def sw(key):
    """The kernel's swizzle: 16-byte slot s of a 64-byte row with key `key` holds chunk s ^ sw(key)."""
    return ((key >> 2) & 1) << 1


def bank_unit(addr):
    return (addr >> 4) & 15


def patch_shapes(max_pos=128, halo_rows=256, xpad=XPAD):
    """Every ph x pw patch api_conv.hip pick_patch may return for conv_hpipe (its feasibility tests, any map size)."""
    for w in range(4, 33):
        for h in range(1, max_pos // w + 1):
            if (h + 2) * (w + xpad) > halo_rows:
                continue
            if ((max_pos - 1) // w + 2) * (w + xpad) + (max_pos - 1) % w + 2 >= halo_rows:
                continue
            yield h, w


def test_patch_shapes_cover_the_pyramid_levels():
    shapes = set(patch_shapes())
    for s in [(10, 12), (9, 14), (13, 7), (7, 11)]:  # 100x168 / 50x84, 25x42, 13x21, 7x11 (api_conv.hip pick_patch comment)
        assert s in shapes


def test_weight_fragment_reads_conflict_free_and_consistent():
    # the re-pack (hpipe_pack_weights_kernel): slot s of stage row r holds chunk s ^ sw(r)
    chunk_at = {(r, s): s ^ sw(r) for r in range(256) for s in range(4)}
    for wn, j in itertools.product(range(4), range(4)):
        addr = {}
        for l in range(64):
            l15, lq = l & 15, l >> 4
            off_b = (wn * 64 + l15) * 64 + ((lq ^ sw(l15)) << 4)  # the kernel's offB (sw of l15 == sw of the full row)
            a = off_b + j * 1024
            row, slot = a // 64, (a % 64) // 16
            assert row == wn * 64 + j * 16 + l15
            assert chunk_at[(row, slot)] == lq, (wn, j, l)
            addr[l] = a
        for g in GROUPS:
            units = {bank_unit(addr[l]) for l in g}
            assert len(units) == 16, (wn, j, g)


@pytest.mark.parametrize("shape", sorted(patch_shapes()), ids=lambda s: f"{s[0]}x{s[1]}")
def test_halo_fragment_reads_conflict_free_and_consistent(shape):
    ph, pw = shape
    hp = pw + XPAD
    inv_pw = (65536 + pw - 1) // pw
    for wm, buf in itertools.product(range(2), range(2)):
        a0 = {}
        for i, l15 in itertools.product(range(8), range(16)):
            m = i * 16 + l15
            my = (m * inv_pw) >> 16
            assert my == m // pw
            a0[i, l15] = (wm * HPROWS + my * hp + (m - my * pw)) * 64
        for t in range(9):
            kh, kw = divmod(t, 3)
            base = HALO_OFF + buf * HBUF + (kh * hp + kw) * 64
            for i in range(8):
                addr = {}
                for l in range(64):
                    l15, lq = l & 15, l >> 4
                    so = (lq ^ sw(l15 + kh * pw + kw)) << 4
                    a = base + a0[i, l15] + so
                    # the halo load put chunk s ^ sw(hy * pw + hx) into slot s of halo row h = hy * hp + hx
                    h = (a - HALO_OFF - buf * HBUF) // 64 - wm * HPROWS
                    hy, hx = divmod(h, hp)
                    m = i * 16 + l15
                    assert (hy, hx) == (m // pw + kh, m % pw + kw)
                    assert 0 <= h < HPROWS
                    slot = (a % 64) // 16
                    assert slot ^ sw(hy * pw + hx) == lq, (shape, wm, t, i, l)
                    addr[l] = a
                for g in GROUPS:
                    units = {bank_unit(addr[l]) for l in g}
                    assert len(units) == 16, (shape, wm, t, i, g)


def test_old_swizzle_is_two_way_on_the_16x16x32_read():
    """The 32x32x16 kernel's weight swizzle, chunk ^ ((r >> 2) & 3), puts two lanes of one group on one bank unit for the
    16x16x32 read pattern: the reason the images were re-derived."""
    worst = 0
    for g in GROUPS:
        units = [(l & 15 & 3) * 4 + ((l >> 4) ^ (((l & 15) >> 2) & 3)) for l in g]
        worst = max(worst, max(units.count(u) for u in units))
    assert worst == 2
