// The core the head's streaming kernels share: GroupNorm + ReLU of a raw bf16 tower output on its way from HBM into MFMA operand
// registers.  gn_logits_kernel, gn_logits_sets_kernel, gn_taps_kernel, gn_cond3x3_kernel (head_fused.hip) and logits_scan_kernel
// (detect.hip) walk the 128-row tile table in 32-row groups, keep the (a, b) coefficients of the wave's current segment in a wave-private
// LDS table and turn a row's 512 bytes into bf16(relu(fma(x, a, b))) 16 bytes per k-step.  "Operand values, K order and rounding points
// are gn_logits_kernel's" in those kernels' comments means: they are the functions below.  Device code only.
#pragma once
#include "gfx950.h"

namespace sylph {

// The (a, b) coefficients of segment seg, coef[seg][256], into a wave's 512-float table: (a0, a1, b0, b1) per channel pair, the order
// gn_relu_x8 reads them in.  Same-wave LDS traffic is ordered: no barrier between this and the reads.
__device__ __forceinline__ void gn_load_coef(float* cfw, const float2* __restrict__ coef, int seg, int lane) {
  const float2* cp = coef + (size_t)seg * 256;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int pr = lane + 64 * i;  // channel pair
    const float2 c0 = cp[2 * pr], c1 = cp[2 * pr + 1];
    *reinterpret_cast<float4*>(&cfw[4 * pr]) = make_float4(c0.x, c1.x, c0.y, c1.y);
  }
}

// bf16x2(relu(fma(x, a, b))) on one packed pair of channels.  The fma is the explicit builtin: detect.hip is compiled with
// -ffp-contract=off and head_fused.hip is not, and this is what makes the two agree.  ReLU acts on the rounded bf16 pair.
__device__ __forceinline__ unsigned gn_relu_pair(unsigned x, f32x2 a, f32x2 b) {
  const f32x2 xf = {__uint_as_float(x << 16), __uint_as_float(x & 0xffff0000u)};
  const f32x2 r = __builtin_elementwise_fma(xf, a, b);
  bf16x2 pk;
  pk[0] = (bf16_t)r[0];
  pk[1] = (bf16_t)r[1];
  const s16x2 z = {0, 0};
  return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(s16x2, pk), z));
}

// the 8 channels 16 ks + 8 lh .. + 7 of a lane's row (k-step ks, k half lh), coefficients from the wave's table
__device__ __forceinline__ u32x4 gn_relu_x8(u32x4 x, const float* cfw, int ks, int lh) {
  const float* cq = cfw + (ks * 16 + lh * 8) * 2;  // 4 channel pairs x (a0, a1, b0, b1)
  u32x4 y;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float4 c4 = *reinterpret_cast<const float4*>(cq + 4 * e);
    y[e] = gn_relu_pair(x[e], f32x2{c4.x, c4.y}, f32x2{c4.z, c4.w});
  }
  return y;
}

// Row group g of a 128-row tile table: group g & 3 of tile g >> 2.  Lane l31 = lane & 31 owns row r0 + l31 of the segment's map.  The
// lane's part is computed on demand, behind the wave-uniform empty() test: computed in front of it, the load of out_row0 moves ahead of
// the branch and the register allocation of every kernel changes (profiles/head_stream_core_isa.txt).
struct RowGroup {
  int seg, r0, nrows;  // segment, first map-relative row of the group, rows of the map
  const SegDesc* sd;
  __device__ __forceinline__ bool empty() const { return r0 >= nrows; }                // wave-uniform: the group lies past a short level
  __device__ __forceinline__ bool valid(int l31) const { return r0 + l31 < nrows; }   // the lane's row lies inside the map
  // the lane's global row; past the map, the map's last row (loaded and computed, never stored)
  __device__ __forceinline__ size_t grow(int l31) const { return (size_t)(sd->out_row0 + (valid(l31) ? r0 + l31 : nrows - 1)); }
};
__device__ __forceinline__ RowGroup row_group(const SegDesc* __restrict__ segs, const int2* __restrict__ tiles, int g) {
  const int2 tl = tiles[g >> 2];
  const int seg = tl.x, r0 = tl.y + (g & 3) * 32;
  const SegDesc& sd = segs[seg];
  return {seg, r0, sd.out_H * sd.out_W, &sd};
}

}  // namespace sylph
