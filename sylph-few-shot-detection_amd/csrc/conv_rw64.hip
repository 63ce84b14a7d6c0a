// 3x3 stride-1 convolution 64 -> 64 channels + FrozenBN [+ residual] + ReLU with the WEIGHTS IN REGISTERS: every res2 conv of the
// BasicBlock ResNets (detectron2 BasicBlock.conv1 / conv2 of R-18 / R-34 at the call site
// sylph/modeling/meta_arch/meta_one_stage_detector.py:181,273), 4 / 6 launches over the largest activation of the network.
//
// On conv_igemm's halo mode every 128-position tile streams the layer's 73.7 KB of weights from L2 into LDS again (conv_rw3.hip's
// header prices that at 128 -> 128).  At 64 -> 64 the WHOLE layer is 72 MFMA fragments = 288 registers per lane, what conv_rw3 holds
// for half of its layer, so here every wave keeps all 64 output channels:
//
//   * ONE persistent 256-thread block per CU, one wave per SIMD.  Weight fragment f = 2 k + h (k-step k = tap * 4 + ks, channel half h)
//     lives in AGPR f for f < 64 (inline-asm MFMA with an AGPR operand, gfx950.h) and in VGPRs for the last four k-steps.
//   * a patch is <= 256 positions (pick_patch), wave w owns positions 64 w .. 64 w + 63 as two 32-row tiles: four accumulators, and
//     every activation fragment read from LDS feeds TWO MFMAs (conv_rw3: one) -- half the LDS read traffic per FLOP.
//   * LDS holds only activations: the (ph + 2) x (pw + 2) input halo, pixels padded to 144 bytes (bottleneck64's pitch) and rows of
//     pixels to a pitch == 9 pw (mod 16) 16-byte units, which puts position m in bank group 9 m (mod 16): distinct over every 16
//     consecutive positions (the rw_row_pitch rule for this pixel pitch).  Double-buffered; the next patch's halo travels through
//     registers (buffer loads issued early in the K loop, written to the other buffer behind the stores).
//   * the residual is the block's INPUT tensor: its 128-byte rows are fetched with the same whole-line buffer loads in front of the K
//     loop and parked in the wave's own rows of the store staging tile a third of the way through it; the epilogue reads them there in
//     the accumulator layout, so it never waits for HBM.
//   * epilogue: v = fma(acc, scale, shift) [+ residual] -> ReLU -> bf16 into the staging tile [256][144 B]; a wave stages only its own
//     64 positions (it holds all their channels), so ONE barrier per patch is enough; stores are whole 128-byte lines, 8 lanes each.
//   * image padding, ragged patches and the step past the last patch are out-of-range buffer offsets: loads return zeros, stores are
//     dropped.  The descriptors carry the tensor's real size (< 4 GiB; the builder falls back to the generic route past that), every
//     offset is computed in full in the vector offset.
//
// Numerics: bf16 operands, fp32 accumulation over the taps in tap order, v = acc * scale + shift (one fma), + residual, ReLU, bf16: the
// rounding points of conv_igemm's halo mode (oracle/bf16.py conv_epilogue).
#include <type_traits>
#include <utility>

#include "gfx950.h"

namespace sylph {

namespace {
template <int B, int E, typename F> __device__ __forceinline__ void static_for(F&& f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    static_for<B + 1, E>(f);
  }
}
constexpr int R6_PP = 144;                      // halo pixel pitch: 128 B of channels + 16 B pad
constexpr int R6_HB = 53248;                    // one halo buffer
constexpr int R6_STG = 2 * R6_HB;               // store staging [256 positions][144 B]
constexpr int R6_BN = R6_STG + 256 * R6_PP;     // scale[64] | shift[64] fp32
constexpr int R6_LDS = R6_BN + 2 * 64 * 4;      // 143 872
static_assert(R6_LDS <= 160 * 1024, "LDS budget");
constexpr int R6_NPC = 11;                      // 16-byte halo pieces per thread: 32 pixels x 8 pieces per pass, <= 352 halo pixels
constexpr unsigned R6_OOB = 0xffffff00u;        // a byte offset no tensor reaches (+ < 256): loads return zeros there, stores are dropped

// LDS pitch of a halo ROW OF PIXELS in bytes: == 9 pw (mod 16) 16-byte units (see the header)
__host__ __device__ inline int r6_row_pitch(int pw) {
  const int k0 = (pw + 2) * (R6_PP / 16);
  return (k0 + ((9 * pw - k0) & 15)) * 16;
}
}  // namespace

template <bool RES> __global__ __launch_bounds__(256, 1) void conv_rw64_kernel(const ConvRw64Args a) {
  typedef bf16_t T;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, lh = lane >> 5;
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, a.bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc(a.y, 0, a.bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(RES ? a.res : a.x), 0, a.bytes, 0x00020000);

  // ---- the layer's weights -> registers: fragment f = 2 k + h holds output channel 32 h + l31, input channels 16 ks + 8 lh .. of tap k / 4 ----
  bf16x8 Wa[64], Wv[8];
  {
    const T* wp = a.w + ((size_t)l31 * 9 * 64 + lh * 8);  // [Cout][3][3][Cin]: tap * 64 + ks * 16 == k * 16
#pragma unroll
    for (int f = 0; f < 64; ++f) Wa[f] = *reinterpret_cast<const bf16x8*>(wp + (f & 1) * (32 * 9 * 64) + (f >> 1) * 16);
#pragma unroll
    for (int f = 0; f < 8; ++f) Wv[f] = *reinterpret_cast<const bf16x8*>(wp + (f & 1) * (32 * 9 * 64) + (32 + (f >> 1)) * 16);
    float* bn = reinterpret_cast<float*>(smem + R6_BN);
    if (tid < 128) bn[tid] = tid < 64 ? a.scale[tid] : a.shift[tid - 64];
  }
  wait_vmcnt<0>();

  // persistent tile walk: blocks of one XCD (blockIdx & 7) take neighbouring patches at the same time
  const int G = gridDim.x, xcd = blockIdx.x & 7, jb = blockIdx.x >> 3, gx = (G + 7) >> 3;
  const int chunk = (a.n_tiles + 7) >> 3;
  auto tile_of = [&](int it) { const int q = it * gx + jb; return __builtin_amdgcn_readfirstlane(q < chunk ? xcd * chunk + q : a.n_tiles); };
  auto load_tile = [&](int t) {
    i32x8 v;
    const BkTile* p = a.bk + t;
    asm volatile("s_load_dwordx8 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(p));
    return v;
  };
  auto relu_pk = [](unsigned u) {
    const s16x2 z = {0, 0};
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(s16x2, u), z));
  };
  auto pack2 = [](float lo, float hi) {
    bf16x2 v;
    v[0] = (bf16_t)lo;
    v[1] = (bf16_t)hi;
    return __builtin_bit_cast(unsigned, v);
  };

  int t = tile_of(0);
  if (t >= a.n_tiles) return;
  i32x8 td = load_tile(t);
  const int PW = td[5], PH = td[4], HW2 = PW + 2, NH = (PH + 2) * HW2, NPOS = PH * PW;  // (every patch of a launch has the same ph x pw)
  const int PY = r6_row_pitch(PW), IH = td[1], IW = td[2];
  const unsigned inv_pw = (unsigned)td[6], inv_hw2 = (unsigned)td[7];
  // piece j of this thread: 16-byte chunk c = tid & 7 of halo pixel q = 32 j + (tid >> 3), row hy = q / (pw + 2): its byte offset in x
  // (R6_OOB outside the image, past the halo, or when there is no such patch) and in a halo buffer (idle pieces land in pixel 0's pad)
  auto halo_goff = [&](int j, const i32x8 d, bool live) {
    const int q = j * 32 + (tid >> 3), hy = (int)(((unsigned)q * inv_hw2) >> 16), hx = q - hy * HW2;
    const int iy = (d[3] >> 16) - 1 + hy, ix = (d[3] & 0xffff) - 1 + hx;
    const bool in = live && q < NH && (unsigned)iy < (unsigned)IH && (unsigned)ix < (unsigned)IW;
    return in ? (unsigned)(d[0] + iy * IW + ix) * 128u + (unsigned)((tid & 7) * 16) : R6_OOB;
  };
  auto halo_loff = [&](int j) {
    const int q = j * 32 + (tid >> 3), hy = (int)(((unsigned)q * inv_hw2) >> 16), hx = q - hy * HW2;
    return q < NH ? hy * PY + hx * R6_PP + (tid & 7) * 16 : 128;
  };
  // row r = 8 j + (lane >> 3) of this wave's 64 positions, 16-byte chunk lane & 7: byte offset in y / the residual (R6_OOB: no such pixel)
  auto pos_off = [&](int j, const i32x8 d) {
    const int m = wave * 64 + j * 8 + (lane >> 3);
    const int my = (int)(((unsigned)m * inv_pw) >> 16), mx = m - my * PW;
    const int oy = (d[3] >> 16) + my, ox = (d[3] & 0xffff) + mx;
    const bool pv = m < NPOS && oy < IH && ox < IW;
    return pv ? (unsigned)(d[0] + oy * IW + ox) * 128u + (unsigned)((lane & 7) * 16) : R6_OOB;
  };
  char* const stg_rows = smem + R6_STG + (wave * 64 + (lane >> 3)) * R6_PP + (lane & 7) * 16;  // row 8 j: + 8 j * R6_PP

  {
    u32x4 h0[R6_NPC];
#pragma unroll
    for (int j = 0; j < R6_NPC; ++j) h0[j] = __builtin_amdgcn_raw_buffer_load_b128(xr, halo_goff(j, td, true), 0, 0);
#pragma unroll
    for (int j = 0; j < R6_NPC; ++j) *reinterpret_cast<u32x4*>(smem + halo_loff(j)) = h0[j];
  }

  for (int it = 0; t < a.n_tiles; ++it) {
    const int t_next = tile_of(it + 1);
    const bool more = t_next < a.n_tiles;
    const i32x8 td_next = load_tile(more ? t_next : t);
    lds_barrier();  // this patch's halo is in buffer it & 1; every wave is done reading the other buffer

    u32x4 rreg[8], hreg[R6_NPC];
    if constexpr (RES) {
#pragma unroll
      for (int j = 0; j < 8; ++j) rreg[j] = __builtin_amdgcn_raw_buffer_load_b128(rr, pos_off(j, td), 0, 0);
    }

    // ===== K loop: acc[2 i + h] = sum over taps and channels of halo(position 64 wave + 32 i + l31 shifted by the tap) x W(half h) =====
    f32x16 acc[4];
    {
      const char* hrow[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int m = wave * 64 + i * 32 + l31;
        const int my = (int)(((unsigned)m * inv_pw) >> 16);
        hrow[i] = smem + (it & 1) * R6_HB + my * PY + (m - my * PW) * R6_PP + 16 * lh;
      }
      constexpr int D = 3;
      bf16x8 af[D][2];
      auto rd = [&](auto kc) {  // the two activation fragments of k-step k = tap * 4 + ks
        constexpr int k = decltype(kc)::value, tap = k >> 2, ks = k & 3, kh = tap / 3, kw = tap - 3 * kh;
        const char* const* hr = hrow;
        bf16x8(*f)[2] = af;
#pragma unroll
        for (int i = 0; i < 2; ++i) f[k % D][i] = *reinterpret_cast<const bf16x8*>(hr[i] + kh * PY + kw * R6_PP + ks * 32);
      };
      auto step = [&](auto kc) {
        constexpr int k = decltype(kc)::value;
        if constexpr (k + D - 1 < 36) rd(std::integral_constant<int, k + D - 1>{});
        if constexpr (RES && k == 12) {  // the residual rows -> this wave's rows of the staging tile (its loads were the first of the patch)
          const u32x4* rg = rreg;
#pragma unroll
          for (int j = 0; j < 8; ++j) *reinterpret_cast<u32x4*>(stg_rows + j * 8 * R6_PP) = rg[j];
        }
        if constexpr (k == (RES ? 13 : 1)) {  // the next patch's halo -> registers (behind the residual: both sets at once do not fit)
          u32x4* hg = hreg;
#pragma unroll
          for (int j = 0; j < R6_NPC; ++j) hg[j] = __builtin_amdgcn_raw_buffer_load_b128(xr, halo_goff(j, td_next, more), 0, 0);
        }
        bf16x8* f = af[k % D];
        const bf16x8 *wa = Wa, *wv = Wv;  // (asm operands naming an enclosing local directly do not capture it in a generic lambda)
        f32x16* ac = acc;
        static_for<0, 4>([&](auto jc) {
          constexpr int j = decltype(jc)::value, i = j & 1, h = j >> 1, fi = 2 * k + h;
          if constexpr (k == 0) mfma_aw0(ac[2 * i + h], wa[fi], f[i]);
          else if constexpr (fi < 64) mfma_aw(ac[2 * i + h], wa[fi], f[i]);
          else mfma_vw(ac[2 * i + h], wv[fi - 64], f[i]);
        });
      };
      rd(std::integral_constant<int, 0>{});
      rd(std::integral_constant<int, 1>{});
      static_for<0, 36>(step);
      mfma_drain(acc[0], acc[1], acc[2], acc[3]);
    }

    // ===== epilogue: FrozenBN [+ residual] + ReLU -> bf16 -> this wave's rows of the staging tile (row m, piece 4 h + g, half lh) =====
    {
      const float* bn = reinterpret_cast<const float*>(smem + R6_BN) + 4 * lh;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        f32x4 sv[4], bv[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          sv[g] = *reinterpret_cast<const f32x4*>(bn + 32 * h + 8 * g);
          bv[g] = *reinterpret_cast<const f32x4*>(bn + 64 + 32 * h + 8 * g);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          char* row = smem + R6_STG + (wave * 64 + i * 32 + l31) * R6_PP + lh * 8;
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = acc[2 * i + h][4 * g + e] * sv[g][e] + bv[g][e];
            u32x2* p = reinterpret_cast<u32x2*>(row + (4 * h + g) * 16);
            if constexpr (RES) {
              const u32x2 rv = *p;
              v[0] += __uint_as_float(rv[0] << 16); v[1] += __uint_as_float(rv[0] & 0xffff0000u);
              v[2] += __uint_as_float(rv[1] << 16); v[3] += __uint_as_float(rv[1] & 0xffff0000u);
            }
            u32x2 o;
            o[0] = pack2(v[0], v[1]);
            o[1] = pack2(v[2], v[3]);
            if (a.relu) { o[0] = relu_pk(o[0]); o[1] = relu_pk(o[1]); }
            *p = o;
          }
        }
      }
    }
    // ===== stores: whole 128-byte lines, 8 lanes per position; then the next patch's halo -> the other buffer =====
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(stg_rows + j * 8 * R6_PP);
      __builtin_amdgcn_raw_buffer_store_b128(v, yr, pos_off(j, td), 0, 0);
    }
#pragma unroll
    for (int j = 0; j < R6_NPC; ++j) *reinterpret_cast<u32x4*>(smem + ((it + 1) & 1) * R6_HB + halo_loff(j)) = hreg[j];
    t = t_next;
    td = td_next;
  }
}

bool conv_rw64_patch_ok(int ph, int pw) {
  if (ph < 1 || pw < 1 || ph * pw > 256) return false;
  const int PY = r6_row_pitch(pw);
  // every halo piece has a register, the halo fits a buffer, and the fragment reads of the pad positions (m up to 255, bottom-right tap)
  // stay inside it
  return (ph + 2) * (pw + 2) <= R6_NPC * 32 && (ph + 2) * PY <= R6_HB && (255 / pw + 2) * PY + (255 % pw + 2) * R6_PP + 128 <= R6_HB;
}

int launch_conv_rw64(const ConvRw64Args& a, hipStream_t s) {
  static PerDeviceOnce once;
  const int dev = current_device(), ncu = device_cu_count(dev);
  if (!once.run(dev, [] {
        return hipFuncSetAttribute((const void*)conv_rw64_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, R6_LDS) == hipSuccess &&
               hipFuncSetAttribute((const void*)conv_rw64_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, R6_LDS) == hipSuccess;
      }))
    return -7;
  if (a.n_tiles < 1 || a.bytes == 0 || a.bytes > R6_OOB) return -8;
  const int want = (a.n_tiles + 7) & ~7;
  const int grid = want < ncu ? want : (ncu & ~7);
  if (a.res) hipLaunchKernelGGL(conv_rw64_kernel<true>, dim3(grid), dim3(256), R6_LDS, s, a);
  else hipLaunchKernelGGL(conv_rw64_kernel<false>, dim3(grid), dim3(256), R6_LDS, s, a);
  return (int)hipGetLastError();
}

}  // namespace sylph
