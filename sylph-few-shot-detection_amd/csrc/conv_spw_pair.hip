// conv3 + residual of a res3 identity block and conv1 of the NEXT block in one launch (bf16):
//
//     y[pos][n]  = relu( (sum_c t2[pos][c] w3[n][c]) * s3[n] + b3[n] + x[pos][n] )        n < 512, c < 128   (conv_spw.hip's layer)
//     t1[pos][m] = relu( (sum_n y[pos][n] w1[m][n]) * s1[m] + b1[m] )                     m < 128            (the next block's conv1)
//
// As two launches (conv_spw<128, 1> + conv_igemm) the pair moves y three times -- written, read back one launch later, and read again as
// the next block's residual; here the second read never happens: 43 instead of 60 MB per 800 x 1333 image and pair.  Both weight sets
// stay in registers for the whole launch (64 + 64 VGPRs per lane), so LDS holds activations only:
//
//   * ONE persistent 512-thread block per CU walks full-width tiles (PAIR_TILE_ROWS = 64 positions x all 512 channels, res3_pair_tiles.h):
//     t2 and x are read once, not once per N tile through L2.
//   * first GEMM: conv_spw's arithmetic -- the same 32x32x16 MFMAs in the same k order, weights as the A operand (D^T: a lane holds 4
//     consecutive channels), epilogue fma(acc, s3, b3) + residual -> ReLU -> bf16 IN PLACE in the LDS buffer the residual landed in.
//     Wave w owns channels 64 w .. 64 w + 63 = column group w of the buffer: y is bit-identical to conv_spw_kernel<128, 1, true>.
//   * second GEMM: its B operand is the finished bf16 y tile in LDS (what conv_igemm would read from HBM), 16x16x32 MFMAs, wave w owns
//     output channels 16 w .. 16 w + 15; fma(acc, s1, b1) -> ReLU -> bf16 -> staged [64 rows][256 B] in the first 16 KiB of the y
//     buffer of the same tile (its reads are over by then) -> stored as whole lines.
//   * the y buffer is double: the residual of tile T + 1 is in flight from the first GEMM of tile T on, a whole tile ahead.
//   * every wave's vector-memory queue holds ONE kind of traffic, so each wait is an exact vmcnt(0) on traffic issued a tile earlier:
//       waves 0-1  A loader: t2 rows of tile T + 1 -> the 16-KiB A buffer, issued when the first GEMM of tile T is done
//       waves 2-3  residual: x rows of tile T + 1 -> y buffer (T + 1) & 1, issued at the same point
//       waves 4-7  stores: y (16-byte stores, 8 lanes per 128-byte line) under the second GEMM, t1 under the next tile's first GEMM;
//                  they never wait for a store
//     (LDS-DMA, whole lines, swizzle on the source side: piece p of row r at slot p ^ (r & 7), as in conv_spw.hip.)
//   * four barriers per tile: A (first GEMM done, residual landed), B (y in the buffer), C (second GEMM and the y stores have read it),
//     D (t1 staged, next A tile landed).
//   * ragged tiles: rows past the image re-read its last row (pair_tile_load_row) and their stores are masked off (pair_tile_stores);
//     no wait counts stores, so their number need not be constant.
//   * a 64-bit base per image + 32-bit offsets inside it.
//
// LDS: A 16 KiB | s3, b3, s1, b1 5 KiB | y 2 x 64 KiB = 149 KiB.  LDS accesses beside a pending LDS-DMA are ext-vector loads or inline asm
// (gfx950.h).
#include "gfx950.h"
#include "res3_pair_tiles.h"

namespace sylph {

namespace {
constexpr int PT = PAIR_TILE_ROWS;
constexpr int OFF_A = 0, A_BYTES = PT * 256;        // [2 phases of 64 channels][64 rows][128 B]
constexpr int OFF_TAB = OFF_A + A_BYTES;            // s3[512] | b3[512] | s1[128] | b1[128] fp32
constexpr int OFF_Y = OFF_TAB + (2 * 512 + 2 * 128) * 4;
constexpr int Y_BYTES = PT * 1024;                  // [8 column groups of 64 channels][64 rows][128 B]
constexpr int PAIR_LDS = OFF_Y + 2 * Y_BYTES;       // 152 576
static_assert(PT == 64, "the wave tiling below is written for 64-row tiles");
static_assert(PAIR_LDS <= 160 * 1024, "LDS budget");
typedef int i32x4 __attribute__((ext_vector_type(4)));
}  // namespace

__global__ __launch_bounds__(512, 1) void conv_spw_kernel_pair(const PairArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, lh = lane >> 5, l15 = lane & 15, kb = lane >> 4;
  // (the role code below re-derives its lane constants from an opaque copy of `lane` per tile: hoisted out of the tile loop they would
  // not fit beside 128 weight and 64 accumulator registers, and a spilled value is reloaded behind an s_waitcnt vmcnt(0))
  auto opaque_lane = [&]() { int ln = lane; asm volatile("" : "+v"(ln)); return ln; };
  const bool loader = wave < 2, resw = wave == 2 || wave == 3, storer = wave >= 4;
  int t = blockIdx.x;
  const int t_step = gridDim.x;
  if (t >= a.n_tiles) return;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
  auto load_desc = [&](int ti) {
    const PairTile* p = a.tiles + ti;
    i32x4 d;
    asm volatile("s_load_dwordx4 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=&s"(d) : "s"(p));
    return PairTile{d[0], d[1], d[2], 0};
  };

  // ---- both weight sets -> registers.  w3: output channels 64 wave + 32 j + l31, k-step ks = channels 16 ks + 8 lh .. (+7);
  //      w1: output channels 16 wave + l15, k-step ks = y channels 32 ks + 8 kb .. (+7) ------------------------------------------------
  bf16x8 wf[2][8], wg[16];
  {
    const bf16_t* wp = a.w3 + (size_t)(wave * 64 + l31) * 128 + lh * 8;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) wf[j][ks] = *reinterpret_cast<const bf16x8*>(wp + j * 32 * 128 + ks * 16);
    const bf16_t* wq = a.w1 + (size_t)(wave * 16 + l15) * 512 + kb * 8;
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) wg[ks] = *reinterpret_cast<const bf16x8*>(wq + ks * 32);
  }
  {
    float* tabp = reinterpret_cast<float*>(smem + OFF_TAB);
    tabp[tid] = a.s3[tid];
    tabp[512 + tid] = a.b3[tid];
    if (tid < 256) tabp[1024 + tid] = tid < 128 ? a.s1[tid] : a.b1[tid - 128];
  }
  // (the builtin, not inline asm: hipcc must know that the weights have landed, or it waits for them -- vmcnt(0) -- at their first use in
  // the tile loop, every tile)
  __builtin_amdgcn_s_waitcnt(0x0070);  // vmcnt(0) lgkmcnt(0)
  __syncthreads();

  // ---- A loader (waves 0-1): wave q loads the 64-channel phase q of the tile's t2 rows: [64 rows][128 B], 8 instructions of 8 rows ----
  const char* const t2b = reinterpret_cast<const char*>(a.t2);
  auto issue_a = [&](const PairTile& d) {
    const int ln = opaque_lane(), r8 = ln >> 3, s8 = ln & 7;
    const char* base = t2b + (size_t)(unsigned)d.img_row0 * 256 + wave * 128 + ((s8 ^ r8) << 4);
    char* dst = smem + OFF_A + wave * 8192;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const unsigned off = (unsigned)pair_tile_load_row(d, 8 * k + r8) * 256u;
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)(base + off), (lds_ptr_t)(dst + k * 1024), 16, 0, 0);
    }
  };
  // ---- residual (waves 2-3): wave 2 + h loads column groups 4 h .. 4 h + 3 of the tile's x rows into y buffer `buf` ---------------------
  const char* const xb = reinterpret_cast<const char*>(a.x);
  auto issue_res = [&](const PairTile& d, int buf) {
    const int ln = opaque_lane(), r8 = ln >> 3, s8 = ln & 7;
    const char* base = xb + (size_t)(unsigned)d.img_row0 * 1024 + (wave - 2) * 512 + ((s8 ^ r8) << 4);
    char* dst = smem + OFF_Y + buf * Y_BYTES + (wave - 2) * 4 * 8192;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const char* src = base + (unsigned)pair_tile_load_row(d, 8 * k + r8) * 1024u;
#pragma unroll
      for (int cg = 0; cg < 4; ++cg)
        __builtin_amdgcn_global_load_lds((gbl_ptr_t)(src + cg * 128), (lds_ptr_t)(dst + cg * 8192 + k * 1024), 16, 0, 0);
    }
  };
  // ---- stores (waves 4-7) ----------------------------------------------------------------------------------------------------------
  char* const yb = reinterpret_cast<char*>(a.y);
  char* const t1b = reinterpret_cast<char*>(a.t1);
  const int sw = wave - 4;
  auto store_y = [&](const PairTile& d, int buf) {  // column groups 2 sw, 2 sw + 1 of the finished tile: 16-byte stores, 8 lanes per line
    const int ln = opaque_lane(), r8 = ln >> 3, s8 = ln & 7;
    char* const gbase = yb + (size_t)(unsigned)d.img_row0 * 1024 + ((s8 ^ r8) << 4);
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int cg = 2 * sw + (h >> 1), k0 = (h & 1) * 4;
      const unsigned region = lds0 + OFF_Y + buf * Y_BYTES + cg * 8192 + ln * 16;
      u32x4 o[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) asm volatile("ds_read_b128 %0, %1" : "=v"(o[k]) : "v"(region + (k0 + k) * 1024));
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(o[0]), "+v"(o[1]), "+v"(o[2]), "+v"(o[3]));
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int rc = 8 * (k0 + k) + r8;
        if (pair_tile_stores(d, rc)) *reinterpret_cast<u32x4*>(gbase + (unsigned)(d.row0 + rc) * 1024u + cg * 128) = o[k];
      }
    }
  };
  auto store_t1 = [&](const PairTile& d, int buf) {  // rows 16 sw .. 16 sw + 15 of the staged t1 tile: 16 lanes per 256-byte row
    const int ln = opaque_lane(), l15 = ln & 15, kb = ln >> 4;
    const unsigned region = lds0 + OFF_Y + buf * Y_BYTES + sw * 4096 + ln * 16;
    u32x4 o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) asm volatile("ds_read_b128 %0, %1" : "=v"(o[k]) : "v"(region + k * 1024));
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(o[0]), "+v"(o[1]), "+v"(o[2]), "+v"(o[3]));
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int rc = 16 * sw + 4 * k + kb;  // (kb = lane >> 4: the row of this lane's 16-byte piece; staged at slot piece ^ (row & 15))
      if (pair_tile_stores(d, rc))
        *reinterpret_cast<u32x4*>(t1b + (size_t)(unsigned)d.img_row0 * 256 + (unsigned)(d.row0 + rc) * 256u + ((l15 ^ (rc & 15)) << 4)) = o[k];
    }
  };

  // ---- fragment addressing (constant per lane) ----------------------------------------------------------------------------------------
  unsigned aoff[4];  // first GEMM: row l31 (+ 32 i) of a phase, piece 2 ks' + lh
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) aoff[ks] = (unsigned)(l31 * 128 + (((2 * ks + lh) ^ (l31 & 7)) << 4));
  const unsigned tab = lds0 + OFF_TAB;

  // ---- prologue: the first tile's A rows and residual ------------------------------------------------------------------------------
  PairTile cur = load_desc(t), prev = cur;
  bool have_prev = false;
  int b = 0;
  if (loader) { issue_a(cur); wait_vmcnt<0>(); }
  if (resw) issue_res(cur, 0);
  fenced_barrier();  // (barrier D of "tile -1")

  while (true) {
    const int tn = t + t_step;
    const bool next_valid = tn < a.n_tiles;
    const unsigned ybuf = lds0 + OFF_Y + b * Y_BYTES;
    // the previous tile's t1 out of its staging (the other y buffer), under this tile's first GEMM
    if (storer && have_prev) store_t1(prev, b ^ 1);

    // ---- first GEMM: 64 rows x this wave's 64 channels over K = 128 ----------------------------------------------------------------
    // (the fragment reads of both GEMMs are inline asm, double-buffered by hand with counted lgkmcnt: in front of a plain LDS load hipcc
    // puts an s_waitcnt vmcnt(0) against the LDS-DMA that may be pending, which here would wait for this wave's stores or next-tile loads)
    f32x16 acc[2][2];
    {
      bf16x8 fa[2][2];
      auto rd = [&](int s, bf16x8(&f)[2]) {
        const unsigned ad = lds0 + OFF_A + (s >> 2) * 8192 + aoff[s & 3];
        asm volatile("ds_read_b128 %0, %1" : "=v"(f[0]) : "v"(ad));
        asm volatile("ds_read_b128 %0, %1" : "=v"(f[1]) : "v"(ad + 4096));
      };
      rd(0, fa[0]);
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        bf16x8(&f)[2] = fa[s & 1];
        if (s < 7) {
          rd(s + 1, fa[(s + 1) & 1]);
          asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(f[0]), "+v"(f[1]));
        } else {
          asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0]), "+v"(f[1]));
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            if (s == 0) {
              f32x16 z;
#pragma unroll
              for (int r = 0; r < 16; ++r) z[r] = 0.f;
              acc[j][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[j][0], f[i], z, 0, 0, 0);
            } else {
              acc[j][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[j][s], f[i], acc[j][i], 0, 0, 0);  // D^T
            }
          }
      }
    }
    if (resw) wait_vmcnt<0>();  // this tile's residual has landed
    fenced_barrier();  // A: the A buffer is free, the residual is in y buffer b, y buffer b ^ 1 has been stored and its staging read
    if (next_valid && (loader || resw)) {
      const PairTile nx = load_desc(tn);
      if (loader) issue_a(nx);
      else issue_res(nx, b ^ 1);
    }
    // ---- first epilogue, in place (conv_spw.hip, K = 512 form: scale / shift re-read per 8-channel group) ---------------------------
    const int ln1 = opaque_lane(), l31 = ln1 & 31, lh = ln1 >> 5;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const unsigned rg = ybuf + wave * 8192 + (i * 32 + l31) * 128 + lh * 8;
        u32x2 rv[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) asm volatile("ds_read_b64 %0, %1" : "=v"(rv[g]) : "v"(rg + (((4 * j + g) ^ (l31 & 7)) << 4)));
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          f32x4 sc4, sh4;
          const int chw = wave * 64 + j * 32 + 8 * g + 4 * lh;
          asm volatile("ds_read_b128 %0, %1" : "=v"(sc4) : "v"(tab + chw * 4));
          asm volatile("ds_read_b128 %0, %1" : "=v"(sh4) : "v"(tab + (512 + chw) * 4));
          if (g == 0) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(sc4), "+v"(sh4), "+v"(rv[0]), "+v"(rv[1]), "+v"(rv[2]), "+v"(rv[3]));
          else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(sc4), "+v"(sh4));
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = __builtin_fmaf(acc[j][i][4 * g + e], sc4[e], sh4[e]);
          const u32x2 rr = rv[g];
          v[0] += __uint_as_float(rr[0] << 16); v[1] += __uint_as_float(rr[0] & 0xffff0000u);
          v[2] += __uint_as_float(rr[1] << 16); v[3] += __uint_as_float(rr[1] & 0xffff0000u);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
          bf16x2 p0, p1;
          p0[0] = (bf16_t)v[0]; p0[1] = (bf16_t)v[1]; p1[0] = (bf16_t)v[2]; p1[1] = (bf16_t)v[3];
          const u32x2 pk = {__builtin_bit_cast(unsigned, p0), __builtin_bit_cast(unsigned, p1)};
          asm volatile("ds_write_b64 %0, %1" ::"v"(rg + (((4 * j + g) ^ (l31 & 7)) << 4)), "v"(pk) : "memory");
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    fenced_barrier();  // B: y buffer b holds the finished y tile
    if (storer) store_y(cur, b);

    // ---- second GEMM: 64 rows x this wave's 16 channels over K = 512, B operand = the y tile ------------------------------------------
    f32x4 c2[4];
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) c2[rg] = f32x4{0.f, 0.f, 0.f, 0.f};
    {
      const int ln3 = opaque_lane(), l15 = ln3 & 15, kb = ln3 >> 4;
      unsigned boff[2];  // row l15 (+ 16 rg) of column group ks >> 1, piece 4 (ks & 1) + kb
#pragma unroll
      for (int p = 0; p < 2; ++p) boff[p] = (unsigned)(l15 * 128 + (((4 * p + kb) ^ (l15 & 7)) << 4));
      bf16x8 fb[2][4];
      auto rd = [&](int ks, bf16x8(&f)[4]) {
        const unsigned ad = ybuf + (ks >> 1) * 8192 + boff[ks & 1];
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) asm volatile("ds_read_b128 %0, %1" : "=v"(f[rg]) : "v"(ad + rg * 2048));
      };
      rd(0, fb[0]);
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) {
        bf16x8(&f)[4] = fb[ks & 1];
        if (ks < 15) {
          rd(ks + 1, fb[(ks + 1) & 1]);
          asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]));
        } else {
          asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]));
        }
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) c2[rg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wg[ks], f[rg], c2[rg], 0, 0, 0);  // D^T
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    fenced_barrier();  // C: nobody reads the y tile any more
    // ---- second epilogue -> staging [64 rows][256 B] at the start of y buffer b: piece p of row r at slot p ^ (r & 15) -----------------
    const int ln2 = opaque_lane(), l15 = ln2 & 15, kb = ln2 >> 4;
    f32x4 sc1, sh1;  // scale / shift of this lane's 4 channels 16 wave + 4 kb .. (+3)
    asm volatile("ds_read_b128 %0, %1" : "=v"(sc1) : "v"(tab + (1024 + wave * 16 + 4 * kb) * 4));
    asm volatile("ds_read_b128 %0, %1" : "=v"(sh1) : "v"(tab + (1152 + wave * 16 + 4 * kb) * 4));
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(sc1), "+v"(sh1));
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = __builtin_fmaf(c2[rg][e], sc1[e], sh1[e]);
        v[e] = v[e] > 0.f ? v[e] : 0.f;
      }
      bf16x2 p0, p1;
      p0[0] = (bf16_t)v[0]; p0[1] = (bf16_t)v[1]; p1[0] = (bf16_t)v[2]; p1[1] = (bf16_t)v[3];
      const u32x2 pk = {__builtin_bit_cast(unsigned, p0), __builtin_bit_cast(unsigned, p1)};
      const unsigned dst = ybuf + (rg * 16 + l15) * 256 + (((2 * wave + (kb >> 1)) ^ l15) << 4) + (kb & 1) * 8;
      asm volatile("ds_write_b64 %0, %1" ::"v"(dst), "v"(pk) : "memory");
    }
    if (loader) wait_vmcnt<0>();  // the next tile's A rows have landed
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    fenced_barrier();  // D: t1 is staged, the A buffer holds the next tile
    prev = cur;
    have_prev = true;
    if (!next_valid) break;
    t = tn;
    cur = load_desc(t);
    b ^= 1;
  }
  if (storer) store_t1(prev, b);
}

int launch_conv_spw_pair(const PairArgs& a, hipStream_t s) {
  if (a.n_tiles <= 0) return -1;
  static PerDeviceOnce once;
  if (!once.run(current_device(), [] {
        return hipFuncSetAttribute((const void*)conv_spw_kernel_pair, hipFuncAttributeMaxDynamicSharedMemorySize, PAIR_LDS) == hipSuccess;
      }))
    return -7;
  const int n_cu = device_cu_count(current_device());
  const int grid = a.n_tiles < n_cu ? a.n_tiles : n_cu;  // one persistent block per CU
  hipLaunchKernelGGL(conv_spw_kernel_pair, dim3(grid), dim3(512), PAIR_LDS, s, a);
  return (int)hipGetLastError();
}

}  // namespace sylph
