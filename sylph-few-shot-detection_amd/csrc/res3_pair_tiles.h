// Tile table of the res3 block-pair kernel (conv_spw_pair.hip): plain C++, shared by the host builder, the kernel and a stand-alone
// host test (tests/test_res3_pair_cpu.py).  A tile is PAIR_TILE_ROWS consecutive positions of ONE image, all channels wide; the last
// tile of an image is ragged: its rows past the image re-read the image's last row (the loads cannot be predicated) and store nothing.
#pragma once
#include <vector>

#ifdef __HIPCC__
#define SYLPH_PAIR_HD __host__ __device__
#else
#define SYLPH_PAIR_HD
#endif

namespace sylph {

constexpr int PAIR_TILE_ROWS = 64;

// one 16-byte descriptor per tile (s_load_dwordx4): the image's first row in the dense [B][HW][C] tensors, the tile's first row inside
// the image, the image's rows
struct PairTile { int img_row0, row0, seg_rows, pad; };

// the row of the image that row r of the tile LOADS (A operand, residual) ...
SYLPH_PAIR_HD inline int pair_tile_load_row(const PairTile& t, int r) {
  const int p = t.row0 + r;
  return p < t.seg_rows ? p : t.seg_rows - 1;
}
// ... and whether it STORES its two outputs (to row t.row0 + r of the image)
SYLPH_PAIR_HD inline bool pair_tile_stores(const PairTile& t, int r) { return t.row0 + r < t.seg_rows; }

// the tiles of B images of HW positions each, image after image
inline std::vector<PairTile> pair_tiles(int B, int HW) {
  std::vector<PairTile> v;
  for (int b = 0; b < B; ++b)
    for (int r0 = 0; r0 < HW; r0 += PAIR_TILE_ROWS) v.push_back(PairTile{b * HW, r0, HW, 0});
  return v;
}

}  // namespace sylph
