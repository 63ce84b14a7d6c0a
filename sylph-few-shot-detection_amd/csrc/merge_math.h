// The arithmetic both view merges share (merge_views.hip, merge_views_large.hip): the order key of a score, rule 1's way back to source
// coordinates and the overlap test of rule 4 (include/sylph_hip.h, sylph_merge_views).  Both files are built without FMA contraction.
#pragma once
#include "common.h"
#include "kernels.h"

namespace sylph {

// float bits -> unsigned that orders like the float (-0 as +0)
__device__ __forceinline__ unsigned merge_score_key(float s) {
  const unsigned u = __float_as_uint(s);
  if ((u << 1) == 0u) return 0x80000000u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// rule 1: row g = view * max_in + row of the [n_views][max_in] boxes, in source coordinates: flipped (x1, x2) <- (w - x2, w - x1); then
// x += x0, y += y0 -- plain fp32 in that order, no clip
__device__ __forceinline__ float4 merge_source_box(const float* __restrict__ boxes, const MergeView* __restrict__ views, unsigned g, unsigned max_in) {
  const MergeView mv = views[g / max_in];
  const float4 b = *reinterpret_cast<const float4*>(boxes + (size_t)g * 4);
  float x1 = b.x, x2 = b.z;
  if (mv.flip) { x1 = mv.w - b.z; x2 = mv.w - b.x; }
  return make_float4(x1 + mv.x0, b.y + mv.y0, x2 + mv.x0, b.w + mv.y0);
}

// IoU > thr for two boxes of the same class: the arithmetic of nms_overlap (detect.hip)
__device__ __forceinline__ bool merge_overlap(float x1, float y1, float x2, float y2, float iarea, float4 b, float thr) {
  const float xx1 = fmaxf(x1, b.x), yy1 = fmaxf(y1, b.y);
  const float xx2 = fminf(x2, b.z), yy2 = fminf(y2, b.w);
  const float w = fmaxf(0.f, xx2 - xx1), h = fmaxf(0.f, yy2 - yy1);
  const float inter = w * h;
  const float jarea = (b.z - b.x) * (b.w - b.y);
  return inter / (iarea + jarea - inter) > thr;
}

__device__ __forceinline__ unsigned long long merge_shfl_u64(unsigned long long v, int src) {
  const unsigned lo = __shfl((unsigned)(v & 0xffffffffull), src);
  const unsigned hi = __shfl((unsigned)(v >> 32), src);
  return ((unsigned long long)hi << 32) | lo;
}

}  // namespace sylph
