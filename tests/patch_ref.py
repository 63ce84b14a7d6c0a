"""Test-side restatement of the patch geometry that the patch-walking backbone kernels are launched with.  TEST INFRASTRUCTURE: the
product never imports this file, and this file never imports the product (it runs without a GPU and without the library).

Restated here, line by line:
  * pick_patch (csrc/api_conv.hip): the ph x pw patch of an H x W map -- at most max_pos positions, (ph + 2) x (pw + xpad) halo rows
    within halo_rows, the fragment reads of the pad positions inside the halo too -- that minimises the number of patches; ties go to
    the smaller halo, then to pw = 16.  bottleneck64[p]_kernel and conv_rw3_kernel are launched with pick_patch(H, W, 128, 184, 2);
  * conv_rw3_patch_ok with rw_row_pitch and RW_TP / RW_HROWS / RW_NPC (csrc/conv_rw3.hip): the patches conv_rw3_kernel can walk;
  * the conv_rw3 launch rule of pick_conv3_route (csrc/api_backbone.hip): SYLPH_CONV_RW3 = 1 (the default) takes launches of at least
    256 * 120 positions, 2 any launch, 0 none; the tensor must stay below the 2 GiB of a buffer descriptor;
  * the patch table of add_patch_kernel (csrc/api_backbone.hip): per image, rows of patches from the top, patches from the left; the
    last row / column of patches is partial when ph / pw does not divide H / W.

The case tables of tests/test_patch_kernels_gpu.py state, per case, the geometry class it is there for; tests/test_patch_kernels_cpu.py
holds every case to its class with these functions, so a retune of pick_patch that moves a case out of its class fails there by name."""
from collections import namedtuple

RW_TP, RW_HROWS, RW_NPC = 272, 192, 12
RW_HB = RW_HROWS * RW_TP
RW3_MIN_POSITIONS = 256 * 120

# the arguments the fused res2 blocks and conv_rw3 pass to pick_patch
MAX_POS, HALO_ROWS, XPAD = 128, 184, 2


def pick_patch(H, W, max_pos=MAX_POS, halo_rows=HALO_ROWS, xpad=XPAD):
    best_n, bh, bw, best_halo = -1, 8, 16, 0
    for w in range(4, 33):
        h = 1
        while h * w <= max_pos:
            ok = (h + 2) * (w + xpad) <= halo_rows
            ok = ok and ((max_pos - 1) // w + 2) * (w + xpad) + (max_pos - 1) % w + 2 < halo_rows
            if ok:
                n = ((H + h - 1) // h) * ((W + w - 1) // w)
                halo = (h + 2) * (w + 2)
                if best_n < 0 or n < best_n or (n == best_n and (halo < best_halo or (halo == best_halo and w == 16))):
                    best_n, bh, bw, best_halo = n, h, w, halo
            h += 1
    return bh, bw


def rw_row_pitch(pw):
    k0 = (pw + 2) * (RW_TP // 16)
    return (k0 + ((pw - k0) & 15)) * 16


def conv_rw3_patch_ok(ph, pw):
    py = rw_row_pitch(pw)
    return (ph * pw <= 128 and ph + 2 <= RW_NPC and pw + 2 <= 16 and (127 // pw + 2) * py + (127 % pw + 2) * RW_TP + 256 <= RW_HB
            and (RW_NPC - 1) * py + (pw + 2) * RW_TP <= RW_HB)


def conv_rw3_route(B, H, W, knob=1):
    """The (ph, pw) conv_rw3_kernel is launched with for a stride-1 128 -> 128 3x3 conv + FrozenBN + ReLU on B maps of H x W (bf16), or
    None where pick_conv3_route leaves the conv to the generic route."""
    pos = B * H * W
    if not knob or pos * 256 >= 1 << 31 or not (knob == 2 or pos >= RW3_MIN_POSITIONS):
        return None
    ph, pw = pick_patch(H, W)
    return (ph, pw) if conv_rw3_patch_ok(ph, pw) else None


Geometry = namedtuple("Geometry", "ph pw tiles_y tiles_x tiles_per_image tiles last_rows last_cols")


def geometry(B, H, W, max_pos=MAX_POS, halo_rows=HALO_ROWS, xpad=XPAD):
    """The patch table of B maps of H x W: the patch, tiles per image and in the launch, and the rows / columns of the map inside the
    last row / column of patches (== ph / pw where the patches divide the map)."""
    ph, pw = pick_patch(H, W, max_pos, halo_rows, xpad)
    ty, tx = (H + ph - 1) // ph, (W + pw - 1) // pw
    return Geometry(ph, pw, ty, tx, ty * tx, B * ty * tx, H - (ty - 1) * ph, W - (tx - 1) * pw)


def classes(B, H, W):
    """The geometry classes of a launch, as the set of their names:
      ragged_y / ragged_x   the last row / column of patches is partial
      exact                 neither
      narrow / short        the map is narrower / lower than ONE patch (the whole patch row or column is partial)
      few_tiles             fewer than 8 tiles: some of the 8 XCD walks of the persistent kernels get none
      odd_walk              a tile count that is not a multiple of 8: the walks have unequal lengths
      second_patch          more than 256 tiles: a persistent block (one per CU, 256 of them) takes a second patch"""
    g = geometry(B, H, W)
    out = set()
    if g.last_rows != g.ph:
        out.add("ragged_y")
    if g.last_cols != g.pw:
        out.add("ragged_x")
    if not out:
        out.add("exact")
    if W < g.pw:
        out.add("narrow")
    if H < g.ph:
        out.add("short")
    if g.tiles < 8:
        out.add("few_tiles")
    if g.tiles % 8:
        out.add("odd_walk")
    if g.tiles > 256:
        out.add("second_patch")
    return out


def patch_edges(y, x, ph, pw, H, W):
    """Where position (y, x) of an H x W map lies in its ph x pw patch: the names among first_row / last_row / first_col / last_col
    (last: of the patch's part inside the map), "" for an interior position."""
    y0, x0 = y - y % ph, x - x % pw
    names = []
    if y == y0:
        names.append("first_row")
    if y == min(y0 + ph, H) - 1:
        names.append("last_row")
    if x == x0:
        names.append("first_col")
    if x == min(x0 + pw, W) - 1:
        names.append("last_col")
    return "+".join(names)
