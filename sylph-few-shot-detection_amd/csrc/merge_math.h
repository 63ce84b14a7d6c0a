// The arithmetic decode NMS and the view merges share (detect.hip, merge_views.hip, merge_views_large.hip, through nms_walk.h): the order
// key of a score, rule 1's way back to source coordinates, the overlap test of NMS and of rule 4 (include/sylph_hip.h, sylph_merge_views),
// the 64-bit shuffle and the tests of the stitching merge (sylph_stitch_views).  All three files are built without FMA contraction.
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

// IoU > thr for two boxes of the same class: torchvision's nms arithmetic (inter / (area_i + area_j - inter), no +1)
__device__ __forceinline__ bool merge_overlap(float x1, float y1, float x2, float y2, float iarea, float4 b, float thr) {
  const float xx1 = fmaxf(x1, b.x), yy1 = fmaxf(y1, b.y);
  const float xx2 = fminf(x2, b.z), yy2 = fminf(y2, b.w);
  const float w = fmaxf(0.f, xx2 - xx1), h = fmaxf(0.f, yy2 - yy1);
  const float inter = w * h;
  const float jarea = (b.z - b.x) * (b.w - b.y);
  return inter / (iarea + jarea - inter) > thr;
}

// The stitching merge (include/sylph_hip.h, sylph_stitch_views).  Rule 0: does a border of its crop that lies inside the source cut the
// box (source coordinates)?  The crop's sides are x0, y0, x0 + w, y0 + h in fp32
__device__ __forceinline__ bool stitch_cut(float4 b, MergeView mv, StitchView sv, float border) {
  const float L = mv.x0, T = mv.y0, R = mv.x0 + mv.w, B = mv.y0 + sv.h;
  return (L > 0.f && b.x <= L + border) || (R < sv.src_w && b.z >= R - border) || (T > 0.f && b.y <= T + border) ||
         (B < sv.src_h && b.w >= B - border);
}

// rule 4a's pair test M(i, j) for two boxes of one class: a pair with a cut box matches on intersection over the smaller box (0 / 0 is
// NaN: no match), any other pair on merge_overlap, which nms_thr <= 0 switches off
__device__ __forceinline__ bool stitch_match(float4 a, float4 b, bool cut_pair, float nms_thr, float stitch_thr) {
  const float aarea = (a.z - a.x) * (a.w - a.y);
  if (!cut_pair) return nms_thr > 0.f && merge_overlap(a.x, a.y, a.z, a.w, aarea, b, nms_thr);
  const float w = fmaxf(0.f, fminf(a.z, b.z) - fmaxf(a.x, b.x)), h = fmaxf(0.f, fminf(a.w, b.w) - fmaxf(a.y, b.y));
  const float inter = w * h;
  const float barea = (b.z - b.x) * (b.w - b.y);
  return inter / fminf(aarea, barea) > stitch_thr;
}

// rule 4b's test: does the union box u hold more than stitch_thr of box b?
__device__ __forceinline__ bool stitch_covered(float4 u, float4 b, float stitch_thr) {
  const float w = fmaxf(0.f, fminf(u.z, b.z) - fmaxf(u.x, b.x)), h = fmaxf(0.f, fminf(u.w, b.w) - fmaxf(u.y, b.y));
  const float inter = w * h;
  return inter / ((b.z - b.x) * (b.w - b.y)) > stitch_thr;
}

__device__ __forceinline__ unsigned long long merge_shfl_u64(unsigned long long v, int src) {
  const unsigned lo = __shfl((unsigned)(v & 0xffffffffull), src);
  const unsigned hi = __shfl((unsigned)(v >> 32), src);
  return ((unsigned long long)hi << 32) | lo;
}

}  // namespace sylph
