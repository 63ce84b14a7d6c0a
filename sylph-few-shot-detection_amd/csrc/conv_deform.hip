// Modulated deformable 3x3 convolution (DCNv2) on MFMA for gfx950: the last conv of a deformable FCOS tower
// (MODEL.FCOS.USE_DEFORMABLE: adet DFConv2d(256, 256, 3, stride 1, padding 1, bias), with_modulated_dcn, deformable_groups 1).
//
//   om = conv3x3(x, offset.weight, offset.bias)        27 channels, fp32 ([rows][om_ld], a separate conv launch: add_conv)
//   tap j = 3 ky + kx:  dy = om[2j], dx = om[2j + 1], mask = sigmoid(om[18 + j])
//   py = float(y - 1 + ky) + dy,  px = float(x - 1 + kx) + dx                                   (fp32)
//   s_j[c] = 0 unless -1 < py < H and -1 < px < W; otherwise the bilinear blend of the neighbours (y0, x0), (y0, x0 + 1),
//            (y0 + 1, x0), (y0 + 1, x0 + 1), y0 = floor(py), x0 = floor(px), a neighbour outside the map contributing 0
//            (detectron2 dmcn_im2col_bilinear); weights w00 = hh hw, w01 = hh lw, w10 = lh hw, w11 = lh lw with
//            lh = py - y0, lw = px - x0, hh = 1 - lh, hw = 1 - lw
//   A[pos][j * 256 + c] = round_T( (((v00 w00 + v01 w01) + v10 w10) + v11 w11) * mask )     fp32, in exactly this order
//   out[pos][n] = bias[n] + sum_k A[pos][k] W[n][k]                                          (+ ReLU, + GroupNorm partials)
//
// Every (image, level) map is its own segment: the four neighbours are addressed inside the output position's segment from a
// 64-bit segment base, so a sample can never read a row of another level or image.  (This file is compiled without FP
// contraction: the blend above is separate multiplies and adds, as tests/deform_ref.py restates it.)
//
// Implicit GEMM: M = output positions (128-row tiles of one segment), N = 256 (one block computes all output channels, so the
// expensive A operand is built once), K = 9 taps x 256 channels walked tap-major in 128-byte slices (64 bf16 / 32 fp32).
// Block = 4 waves (2 x 2), wave tile 64 x 128 of 32x32 MFMAs; the Mma policies and the LDS row swizzle are conv_igemm's
// (igemm_mma.h): bf16 operands in the bf16 mode, exact fp32 MFMAs in the fp32 mode AND in the split-bf16 parity mode (DT_F32S: the
// layer's weights are packed in fp32 for it, api_weights.hip).  A split-bf16 instantiation (MmaSplit) was tried: on the GPU the
// second 32-row M fragment of each wave came out wrong (~20 % relative) while the fp32 and bf16 instantiations of the same loop
// matched; it is not built until that is understood.
//
// Per slice: the weight rows stream HBM/L2 -> LDS by LDS-DMA (global_load_lds_dwordx4) as in conv_igemm; the A slice cannot
// (it is blended in registers): every thread owns one 16-byte chunk of four tile rows, fetches the four neighbour chunks of each
// (16 x 16-byte loads), blends them in fp32 and writes one ds_write_b128 per row into the swizzled slot.  Both are issued for
// slice k + 1 before the MFMAs of slice k (two LDS stages, 96 KiB, one barrier per slice), so the gather's L2 round trip runs
// under the MFMAs.  The per-tap sample table (neighbour offsets, weights, mask) lives in registers; the next tap's three om
// values per row are fetched one tap ahead.
#include "gfx950.h"
#include "igemm_mma.h"
#include "kernels.h"

namespace sylph {

namespace {


constexpr int DBM = 128, DBN = 256, DNT = 256;  // tile rows, output channels, threads
constexpr int DSTAGE = (DBM + DBN) * 128;       // one LDS stage: A rows then weight rows, 128 B each
constexpr int DLDS = 2 * DSTAGE;                // 96 KiB (the fp32 epilogue tile, 64 x 260 floats, aliases it)
constexpr int DKTOT = 9 * 256;

// sample table of one tile row for one tap: element offsets of the four neighbours inside the segment (-1: reads zeros),
// their bilinear weights and the modulation mask
__device__ __forceinline__ void tap_sample(float dy, float dx, float ml, int y, int x, int ky, int kx, int H, int W, bool rv, int (&off)[4],
                                           float (&w)[4], float& m) {
  const float py = (float)(y - 1 + ky) + dy, px = (float)(x - 1 + kx) + dx;
  m = 1.f / (1.f + expf(-ml));
#pragma unroll
  for (int k = 0; k < 4; ++k) { off[k] = -1; w[k] = 0.f; }
  if (rv && py > -1.f && px > -1.f && py < (float)H && px < (float)W) {  // (NaN / inf offsets fail here: no sample)
    const float fy = floorf(py), fx = floorf(px);
    const int y0 = (int)fy, x0 = (int)fx;
    const float lh = py - fy, lw = px - fx, hh = 1.f - lh, hw = 1.f - lw;
    w[0] = hh * hw; w[1] = hh * lw; w[2] = lh * hw; w[3] = lh * lw;
    if (y0 >= 0 && x0 >= 0) off[0] = (y0 * W + x0) * 256;
    if (y0 >= 0 && x0 + 1 < W) off[1] = (y0 * W + x0 + 1) * 256;
    if (y0 + 1 < H && x0 >= 0) off[2] = ((y0 + 1) * W + x0) * 256;
    if (y0 + 1 < H && x0 + 1 < W) off[3] = ((y0 + 1) * W + x0 + 1) * 256;
  }
}

__device__ __forceinline__ void unpack16(const uint4& u, float (&v)[8], bf16_t) {
  v[0] = __uint_as_float(u.x << 16); v[1] = __uint_as_float(u.x & 0xffff0000u);
  v[2] = __uint_as_float(u.y << 16); v[3] = __uint_as_float(u.y & 0xffff0000u);
  v[4] = __uint_as_float(u.z << 16); v[5] = __uint_as_float(u.z & 0xffff0000u);
  v[6] = __uint_as_float(u.w << 16); v[7] = __uint_as_float(u.w & 0xffff0000u);
}
__device__ __forceinline__ void unpack16(const uint4& u, float (&v)[4], float) {
  v[0] = __uint_as_float(u.x); v[1] = __uint_as_float(u.y); v[2] = __uint_as_float(u.z); v[3] = __uint_as_float(u.w);
}
__device__ __forceinline__ uint4 pack16(const float (&v)[8], bf16_t) {
  bf16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (bf16_t)v[e];
  return *reinterpret_cast<const uint4*>(&o);
}
__device__ __forceinline__ uint4 pack16(const float (&v)[4], float) {
  return make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3]));
}

template <typename T>
__global__ __launch_bounds__(DNT, 1) void conv_deform_kernel(const DeformArgs a) {
  constexpr int EPC = 16 / (int)sizeof(T);  // elements per 16-byte chunk
  constexpr int BK = 8 * EPC;               // elements per 128-byte K-slice
  constexpr int CPT = 256 / BK, NK = 9 * CPT;
  constexpr int WTM = 64, WTN = 128, TM = 2, TN = 4;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  // XCD-aware block -> tile map (as conv_igemm.hip): an XCD owns a contiguous run of tiles, i.e. neighbouring rows of a map,
  // whose gathers then share that XCD's L2
  const int xcd = blockIdx.x & 7, q = blockIdx.x >> 3;
  const int chunk = (a.n_mtiles + 7) >> 3;
  const int mt = xcd * chunk + q;
  if (q >= chunk || mt >= a.n_mtiles) return;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int c16 = tid & 7, r0 = tid >> 3;                   // this thread's chunk and first tile row (rows r0 + 32 i)
  const int slot = (c16 ^ ((r0 >> 1) & 7)) << 4;            // LDS byte offset of that chunk in its rows (same for every i)
  const int2 tile = a.tiles[mt];
  const SegDesc sd = a.segs[tile.x];
  const int H = sd.in_H, W = sd.in_W, seg_rows = sd.out_H * sd.out_W;
  const T* __restrict__ xb = reinterpret_cast<const T*>(a.x) + (size_t)sd.in_row0 * 256 + c16 * EPC;  // 64-bit segment base
  const T* __restrict__ zp = reinterpret_cast<const T*>(a.zeros) + c16 * EPC;
  const float* __restrict__ omb = a.om + (size_t)sd.out_row0 * a.om_ld;
  const T* __restrict__ wt = reinterpret_cast<const T*>(a.wt);

  int ry[4], rx[4], rp[4];
  bool rv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int pos = tile.y + r0 + 32 * i;
    rv[i] = pos < seg_rows;
    rp[i] = rv[i] ? pos : 0;
    ry[i] = rp[i] / sd.out_W;
    rx[i] = rp[i] - ry[i] * sd.out_W;
  }
  float omn[4][3];  // (dy, dx, mask logit) of the next tap per row
  auto fetch_om = [&](int t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float* p = omb + (size_t)rp[i] * a.om_ld;
      omn[i][0] = p[2 * t]; omn[i][1] = p[2 * t + 1]; omn[i][2] = p[18 + t];
    }
  };
  int off[4][4];
  float wgt[4][4], msk[4];
  auto set_tap = [&](int t) {
    const int ky = t / 3, kx = t - ky * 3;
#pragma unroll
    for (int i = 0; i < 4; ++i) tap_sample(omn[i][0], omn[i][1], omn[i][2], ry[i], rx[i], ky, kx, H, W, rv[i], off[i], wgt[i], msk[i]);
  };

  // weight rows of the block-wide LDS-DMA: lane (row r0 + 32 j, slot c16) fetches logical chunk c16 ^ ((r0 >> 1) & 7)
  const int bbase = r0 * DKTOT + (c16 ^ ((r0 >> 1) & 7)) * EPC;
  auto issue_w = [&](int buf, int kt) {
    char* dB = smem + buf * DSTAGE + DBM * 128 + wave * 8 * 128;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)(wt + (bbase + j * 32 * DKTOT + kt * BK)), (lds_ptr_t)(dB + j * 32 * 128), 16, 0, 0);
  };
  uint4 va[4][4];
  auto load_a = [&](int cc) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const T* p = off[i][k] >= 0 ? xb + (off[i][k] + cc * BK) : zp;
        va[i][k] = *reinterpret_cast<const uint4*>(p);
      }
  };
  auto write_a = [&](int buf) {
    char* dA = smem + buf * DSTAGE + slot;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v00[EPC], v01[EPC], v10[EPC], v11[EPC], o[EPC];
      unpack16(va[i][0], v00, T()); unpack16(va[i][1], v01, T()); unpack16(va[i][2], v10, T()); unpack16(va[i][3], v11, T());
#pragma unroll
      for (int e = 0; e < EPC; ++e)
        o[e] = (((v00[e] * wgt[i][0] + v01[e] * wgt[i][1]) + v10[e] * wgt[i][2]) + v11[e] * wgt[i][3]) * msk[i];
      *reinterpret_cast<uint4*>(dA + (r0 + 32 * i) * 128) = pack16(o, T());
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  auto compute = [&](int buf) {
    const char* tA = smem + buf * DSTAGE;
    const char* tB = tA + DBM * 128;
#pragma unroll
    for (int ks = 0; ks < Mma<T>::KSTEPS; ++ks) {
      typename Mma<T>::frag_t fa[TM], fb[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) fa[i] = Mma<T>::load(tA, wm * WTM + i * 32 + (lane & 31), ks, lane);
#pragma unroll
      for (int j = 0; j < TN; ++j) fb[j] = Mma<T>::load(tB, wn * WTN + j * 32 + (lane & 31), ks, lane);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = Mma<T>::mma(fb[j], fa[i], acc[i][j]);  // D^T: a lane holds 4 consecutive channels
    }
  };

  // prologue: tap 0's table, slice 0 staged, tap 1's om values in flight
  fetch_om(0);
  set_tap(0);
  fetch_om(1);
  issue_w(0, 0);
  load_a(0);
  wait_vmcnt<0>();
  write_a(0);
  __syncthreads();
  for (int kt = 0; kt < NK; ++kt) {
    const int buf = kt & 1, nk = kt + 1;
    if (nk < NK) {
      const int ntap = nk / CPT, ncc = nk - ntap * CPT;
      if (ncc == 0) {
        set_tap(ntap);
        if (ntap + 1 < 9) fetch_om(ntap + 1);
      }
      issue_w(buf ^ 1, nk);
      load_a(ncc);
    }
    compute(buf);
    if (nk < NK) {
      wait_vmcnt<0>();
      write_a(buf ^ 1);
    }
    __syncthreads();
  }

  // ---- epilogue: bias (+ ReLU), GroupNorm partials of the fp32 values, 16-byte stores (conv_igemm's FAST epilogue for BN = 256)
  float* const sC = reinterpret_cast<float*>(smem);
  constexpr int SCP = DBN + 4, TPR = DBN / 8, RPP = DNT / TPR;
  const int c8 = tid % TPR, rr = tid / TPR, n0 = c8 * 8;
  float sh[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) sh[e] = a.bias[n0 + e];
  float gn_n = 0.f, gn_pv = 0.f, gn_s1 = 0.f, gn_s2 = 0.f;
  T* __restrict__ outn = reinterpret_cast<T*>(a.out) + (size_t)sd.out_row0 * 256 + n0;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    if (p > 0) lds_barrier();
    if (wm == p) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int g = 0; g < 4; ++g)
            *reinterpret_cast<float4*>(sC + (i * 32 + (lane & 31)) * SCP + wn * WTN + j * 32 + 8 * g + 4 * (lane >> 5)) =
                make_float4(acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]);
    }
    lds_barrier();
#pragma unroll
    for (int it = 0; it < WTM / RPP; ++it) {
      const int rl = rr + it * RPP, pos = tile.y + p * WTM + rl;
      if (pos < seg_rows) {
        float v[8];
        const float4 lo = *reinterpret_cast<const float4*>(sC + rl * SCP + n0);
        const float4 hi = *reinterpret_cast<const float4*>(sC + rl * SCP + n0 + 4);
        v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += sh[e];
        if (a.relu) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
        }
        if (a.gn_partial) {
          if (gn_n == 0.f) gn_pv = 0.125f * (((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7])));
#pragma unroll
          for (int e = 0; e < 8; ++e) { const float d = v[e] - gn_pv; gn_s1 += d; gn_s2 += d * d; }
          gn_n += 8.f;
        }
        store8<T>(outn + (size_t)pos * 256, v);
      }
    }
  }
  if (a.gn_partial) gn_tile_reduce<RPP, TPR>(sC, rr, c8, gn_n, gn_pv, gn_s1, gn_s2, a.gn_partial + ((size_t)mt * 32 + c8) * 3, true);
}

template <typename T>
int launch_t(const DeformArgs& a, hipStream_t s) {
  static PerDeviceOnce once;
  auto kern = conv_deform_kernel<T>;
  if (!once.run(current_device(), [&] { return hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, DLDS) == hipSuccess; }))
    return -7;
  const int grid = 8 * ((a.n_mtiles + 7) / 8);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(DNT), DLDS, s, a);
  return (int)hipGetLastError();
}

}  // namespace

int launch_conv_deform(DType dt, const DeformArgs& a, hipStream_t s) {
  if (a.n_mtiles <= 0) return 0;
  if (!a.x || !a.om || !a.wt || !a.bias || !a.out || !a.zeros || a.om_ld < 27) return -1;
  if (dt == DT_BF16) return launch_t<bf16_t>(a, s);
  return launch_t<float>(a, s);  // DT_F32 and DT_F32S: fp32 weights, exact fp32 MFMAs
}

}  // namespace sylph
