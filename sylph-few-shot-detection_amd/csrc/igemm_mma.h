// MFMA operand policies and the per-tile GroupNorm partial reduction shared by the implicit-GEMM conv kernels
// (conv_igemm.hip, conv_deform.hip).  Both kernels stage 128-byte K-slices per LDS row with the 16-byte chunk swizzle
// slot = chunk ^ ((row >> 1) & 7), which is what the fragment readers below undo.
#pragma once
#include "gfx950.h"

namespace sylph {

template <typename T> struct Mma;

template <> struct Mma<bf16_t> {
  static constexpr int KSTEPS = 4;  // 64 bf16 per slice / 16 per MFMA
  typedef bf16x8 frag_t;
  static __device__ __forceinline__ frag_t load(const char* tile, int row, int ks, int lane) {
    const int chunk = ks * 2 + (lane >> 5);
    const int sw = chunk ^ ((row >> 1) & 7);
    return *reinterpret_cast<const frag_t*>(tile + row * 128 + sw * 16);
  }
  static __device__ __forceinline__ frag_t load_sw(const char* tile, int row, int ks, int lane, int swz) {
    return *reinterpret_cast<const frag_t*>(tile + row * 128 + ((ks * 2 + (lane >> 5)) ^ swz) * 16);
  }
  static __device__ __forceinline__ f32x16 mma(frag_t a, frag_t b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
};

template <> struct Mma<float> {
  static constexpr int KSTEPS = 16;  // 32 fp32 per slice / 2 per MFMA
  typedef float frag_t;
  static __device__ __forceinline__ frag_t load(const char* tile, int row, int ks, int lane) {
    const int k = ks * 2 + (lane >> 5);
    const int sw = (k >> 2) ^ ((row >> 1) & 7);
    return *reinterpret_cast<const float*>(tile + row * 128 + sw * 16 + (k & 3) * 4);
  }
  static __device__ __forceinline__ frag_t load_sw(const char* tile, int row, int ks, int lane, int swz) {
    const int k = ks * 2 + (lane >> 5);
    return *reinterpret_cast<const float*>(tile + row * 128 + ((k >> 2) ^ swz) * 16 + (k & 3) * 4);
  }
  static __device__ __forceinline__ f32x16 mma(frag_t a, frag_t b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
  }
};

// Split-bf16 parity mode (DT_F32S): fp32 activations and fp32-sized weights in HBM / LDS exactly as in the fp32 mode, but the products
// run on the bf16 pipe at 3/16 of the fp32-MFMA cost.  x = hi + lo with hi = bf16(x), lo = bf16(x - hi) (both round-to-nearest-even:
// |x - hi - lo| <= 2^-18 |x|), and x * w ~ hi_x hi_w + hi_x lo_w + lo_x hi_w into the same fp32 accumulator (the dropped lo * lo term
// is 2^-18 relative).  Activations are split in registers when a fragment is read (8 consecutive fp32 of one row = two ds_read_b128);
// weights are split ONCE on the host: each 32-element K-slice of a packed row is stored as [32 bf16 hi | 32 bf16 lo] -- the same 128
// bytes, so the staging code does not know the difference.
struct MmaSplit {
  static constexpr int KSTEPS = 2;  // 32 fp32 per slice / 16 per MFMA
  static __device__ __forceinline__ void load_a(const char* tile, int row, int ks, int lane, bf16x8& hi, bf16x8& lo) {
    const int c0 = ks * 4 + (lane >> 5) * 2, sw = (row >> 1) & 7;
    const f32x4 p = *reinterpret_cast<const f32x4*>(tile + row * 128 + ((c0 ^ sw) << 4));
    const f32x4 q = *reinterpret_cast<const f32x4*>(tile + row * 128 + (((c0 + 1) ^ sw) << 4));
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bf16_t hp = (bf16_t)p[e], hq = (bf16_t)q[e];
      hi[e] = hp; hi[4 + e] = hq;
      lo[e] = (bf16_t)(p[e] - (float)hp); lo[4 + e] = (bf16_t)(q[e] - (float)hq);
    }
  }
  static __device__ __forceinline__ void load_w(const char* tile, int row, int ks, int lane, bf16x8& hi, bf16x8& lo) {
    const int c = ks * 2 + (lane >> 5), sw = (row >> 1) & 7;
    hi = *reinterpret_cast<const bf16x8*>(tile + row * 128 + ((c ^ sw) << 4));
    lo = *reinterpret_cast<const bf16x8*>(tile + row * 128 + (((c + 4) ^ sw) << 4));
  }
};

// Per-tile GroupNorm partial: every lane holds shifted sums over its rows of one 8-channel group; the RPP lanes of a
// group are merged (Chan) in a fixed order by lane row 0 and written as (n, mean, M2).
template <int RPP, int TPR>
__device__ __forceinline__ void gn_tile_reduce(float* red, int rr, int c8, float gn_n, float gn_pv, float gn_s1, float gn_s2,
                                               float* gp, bool active) {
  lds_barrier();
  const float inv_n = gn_n > 0.f ? 1.f / gn_n : 0.f;
  red[(rr * TPR + c8) * 3 + 0] = gn_n;
  red[(rr * TPR + c8) * 3 + 1] = gn_pv + gn_s1 * inv_n;          // lane mean
  red[(rr * TPR + c8) * 3 + 2] = gn_s2 - gn_s1 * gn_s1 * inv_n;  // lane M2
  lds_barrier();
  if (rr == 0 && active) {
    float N = 0.f, M = 0.f, Q = 0.f;
    for (int r = 0; r < RPP; ++r) {
      const float nb = red[(r * TPR + c8) * 3 + 0];
      if (nb > 0.f) {
        const float mb = red[(r * TPR + c8) * 3 + 1], qb = red[(r * TPR + c8) * 3 + 2];
        const float nn = N + nb, delta = mb - M;
        M += delta * (nb / nn);
        Q += qb + delta * delta * (N * nb / nn);
        N = nn;
      }
    }
    gp[0] = N; gp[1] = M; gp[2] = Q;
  }
}

}  // namespace sylph
