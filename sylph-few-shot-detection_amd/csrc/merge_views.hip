// Merge of the detections of several VIEWS of one source image (test-time augmentation, tiled inference): gfx950.
// Every view was decoded on its own (sylph_decode_nms with the view's crop size as output size), so its boxes are in crop pixels, in the
// mirrored crop for a flipped view.  One 1024-thread block per source:
//   1  pool: the rows of the source's views in ascending view index, rows in order; key = (ordered score bits << 32) | ~(view * max_in + row)
//   2  bitonic sort of the keys in LDS, descending: by score, ties to the lower view, then to the lower row (the keys are unique)
//   3  boxes back to source coordinates, in sorted order, into LDS: flipped (x1, x2) <- (w - x2, w - x1); then x += x0, y += y0 -- plain
//      fp32 operations in that order, no clip (this file is built without FMA contraction, like detect.hip)
//   4  block_walk (nms_walk.h), the function nms_kernel (detect.hip) runs, over the sorted pool in chunks of 64 boxes: ballots against the
//      boxes kept in earlier chunks, a 64 x 64 bit matrix inside the chunk, a serial resolve in wave 0; same overlap arithmetic, same
//      post-NMS keep rule
//   5  emit: box, score, class and the (view, row) the detection came from
// Nothing is kept between calls and no atomic touches global memory.
#include "common.h"
#include "kernels.h"
#include "nms_walk.h"

namespace sylph {

// what block_walk (nms_walk.h) asks of the pool in LDS: sorted position p holds row ~(low word of keys[p]); the box goes out as it is
struct MergeWalkSrc {
  const unsigned long long* keys;
  const float4* s_box;
  const int* s_cls;
  const float* scores;
  int max_in;
  float *out_boxes, *out_scores;
  int *out_classes, *out_view, *out_row;
  __device__ __forceinline__ unsigned row(unsigned p) const { return ~(unsigned)(keys[p] & 0xffffffffull); }
  __device__ __forceinline__ float4 box(unsigned p) const { return s_box[p]; }
  __device__ __forceinline__ int cls(unsigned p) const { return s_cls[p]; }
  __device__ __forceinline__ float score(unsigned p) const { return scores[row(p)]; }
  __device__ __forceinline__ bool shape(float4&) const { return true; }
  __device__ __forceinline__ void write(size_t o, unsigned p, float4 b, float score, int cls) const {
    const unsigned g = row(p);
    out_boxes[o * 4 + 0] = b.x; out_boxes[o * 4 + 1] = b.y; out_boxes[o * 4 + 2] = b.z; out_boxes[o * 4 + 3] = b.w;
    out_scores[o] = score;
    out_classes[o] = cls;
    out_view[o] = (int)(g / (unsigned)max_in);
    out_row[o] = (int)(g % (unsigned)max_in);
  }
};

// dynamic LDS: keys [pool_p2] u64 | boxes [pool_p2] float4 | classes [pool_p2] int | view prefix [max_views + 1] int | kept [pool_p2] u16
__global__ __launch_bounds__(1024) void merge_views_kernel(const int* __restrict__ src_off, const int* __restrict__ src_views,
                                                           const MergeView* __restrict__ views, int pool_p2, int max_views, int max_in,
                                                           const float* __restrict__ boxes, const float* __restrict__ scores,
                                                           const int* __restrict__ classes, const int* __restrict__ counts, float thr, int K,
                                                           int max_out, float* out_boxes, float* out_scores, int* out_classes, int* out_view,
                                                           int* out_row, int* out_counts, int* status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char merge_lds[];
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(merge_lds);
  float4* s_box = reinterpret_cast<float4*>(merge_lds + (size_t)8 * pool_p2);
  int* s_cls = reinterpret_cast<int*>(merge_lds + (size_t)24 * pool_p2);
  int* s_pref = s_cls + pool_p2;
  unsigned short* kept_pos = reinterpret_cast<unsigned short*>(s_pref + max_views + 1);
  __shared__ BlockWalkLds s_walk;
  const int src = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int v0 = src_off[src], nv = min(src_off[src + 1] - v0, max_views);
  // 1: rows per view (a count outside [0, max_in] is clamped), their prefix, the keys
  for (int i = t; i < nv; i += 1024) {
    const int cn = counts[src_views[v0 + i]];
    s_pref[i + 1] = cn < 0 ? 0 : (cn > max_in ? max_in : cn);
  }
  if (t == 0) s_pref[0] = 0;
  __syncthreads();
  if (t == 0)
    for (int i = 0; i < nv; ++i) s_pref[i + 1] += s_pref[i];
  __syncthreads();
  const unsigned n = min((unsigned)s_pref[nv], (unsigned)pool_p2);  // (the host has checked nv * max_in <= pool_p2)
  unsigned P = 64;
  while (P < n) P <<= 1;
  for (unsigned i = t; i < P; i += 1024) {
    unsigned long long key = 0ull;  // below every real key
    if (i < n) {
      int lo = 0, hi = nv - 1;  // the view whose rows hold pool position i: last k with s_pref[k] <= i
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((unsigned)s_pref[mid] <= i) lo = mid; else hi = mid - 1;
      }
      const unsigned g = (unsigned)src_views[v0 + lo] * (unsigned)max_in + (i - (unsigned)s_pref[lo]);
      key = ((unsigned long long)merge_score_key(scores[g]) << 32) | (unsigned long long)(~g);
    }
    keys[i] = key;
  }
  __syncthreads();
  // 2: bitonic network over P >= 64 keys (P a power of two; the pool itself is any size: the padding keys sort to the end)
  for (unsigned size = 2; size <= P; size <<= 1) {
    for (unsigned stride = size >> 1; stride > 0; stride >>= 1) {
      for (unsigned u = t; u < (P >> 1); u += 1024) {
        const unsigned lo = ((u / stride) * (stride << 1)) + (u % stride);
        const unsigned hi = lo + stride;
        const bool desc = ((lo & size) == 0);
        const unsigned long long a = keys[lo], b = keys[hi];
        if ((a < b) == desc) { keys[lo] = b; keys[hi] = a; }
      }
      __syncthreads();
    }
  }
  // 3: boxes in source coordinates, classes, in sorted order
  for (unsigned i = t; i < n; i += 1024) {
    const unsigned g = ~(unsigned)(keys[i] & 0xffffffffull);
    s_box[i] = merge_source_box(boxes, views, g, (unsigned)max_in);
    s_cls[i] = classes[g];
  }
  // 4 + 5 (the walk's first barrier ends step 3)
  const MergeWalkSrc wsrc = {keys, s_box, s_cls, scores, max_in, out_boxes, out_scores, out_classes, out_view, out_row};
  bool truncated;
  const int nout = block_walk(s_walk, kept_pos, n, thr, K, max_out, wsrc, &truncated);
  if (wave == 0) {
    if (__any(truncated) && lane == 0) *status = 2;  // (every truncated source stores the same word: no atomic)
    if (lane == 0) out_counts[src] = nout < max_out ? nout : max_out;
  }
}

int launch_merge_views(int n_src, const int* src_off, const int* src_views, const MergeView* views, int max_views_per_src, int pool_max,
                       int max_in, const float* boxes, const float* scores, const int* classes, const int* counts, float nms_thresh,
                       int post_nms_topk, int max_out, float* out_boxes, float* out_scores, int* out_classes, int* out_view, int* out_row,
                       int* out_counts, int* status, hipStream_t s) {
  if (n_src <= 0 || pool_max < 0 || pool_max > MERGE_POOL_CAP || max_in <= 0 || max_out <= 0 || max_views_per_src < 0) return (int)hipErrorInvalidValue;
  int p2 = 64;
  while (p2 < pool_max) p2 <<= 1;
  // keys 8 + boxes 16 + classes 4 + kept 2 bytes per pool slot, the view prefix in between (4-byte aligned: the kept positions are u16)
  const size_t lds = (size_t)30 * p2 + (size_t)4 * (max_views_per_src + 1);
  constexpr int LDS_MAX = 30 * MERGE_POOL_CAP + 4 * (MERGE_POOL_CAP + 1);  // 139 268 B of the CU's 160 KiB
  static PerDeviceOnce once;
  if (!once.run(current_device(), [] {
        return hipFuncSetAttribute((const void*)merge_views_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX) == hipSuccess;
      }))
    return -7;
  if (hipMemsetAsync(status, 0, sizeof(int), s) != hipSuccess) return -8;
  hipLaunchKernelGGL(merge_views_kernel, dim3(n_src), dim3(1024), lds, s, src_off, src_views, views, p2, max_views_per_src, max_in, boxes, scores,
                     classes, counts, nms_thresh, post_nms_topk, max_out, out_boxes, out_scores, out_classes, out_view, out_row, out_counts, status);
  return (int)hipGetLastError();
}

}  // namespace sylph
