// LVIS (federated) bbox matching on the device (lvis-api's LVISEval.evaluate_img for iou_type "bbox"): gfx950.
// All arithmetic that reaches a result is float64 in the order of tests/lviseval_ref.py; this file is built without FMA contraction.
// The accumulation is coco_accumulate_kernel (coco_eval.hip) with one unbounded maxDet.
//
// lvis_match_kernel: one wave per EXISTING (image, category) pair -- the caller passes the compacted pair list (pair_cat, pair_flags,
// det_off, gt_off), never a table of images x categories.  The grid is sized from a host-known upper bound of the pair count; the live
// count is a device scalar and the surplus waves return.  LVIS_MATCH_WAVES waves share a block but nothing else: each has an LDS slice of
// LVIS_MATCH_SLICE_BYTES and synchronises only with itself (no block barrier: waves leave at different times).
//   1  detection boxes XYXY fp32 -> XYWH float64 in the slice; per ground-truth box a 64-byte state row: bytes 0..39 "matched at (area,
//      threshold) lane", byte 63 = ignored-in-area-range bits (the annotation's ignore flag, or its area outside the range)
//   2  when lvis_match_fits(D, G) -- the pair's OWN counts -- the D x G IoU tile, float64, into the slice; otherwise no tile: the IoU is
//      recomputed at every visit and the state rows live in the caller's scratch.  Same expression, same bits.
//   3  the greedy walk: lane a * T + t owns (area range a, threshold t) and walks the detections in order (score descending, no cut); per
//      detection the non-ignored boxes in file order, then -- only while unmatched -- the ignored ones.  A matched box is never matched again
//      (LVIS has no crowd boxes).  An unmatched detection is ignored when its own area is outside the range or the pair's category is not
//      exhaustively annotated in the image (pair_flags bit 0)
//   4  per detection two ballots give the 40-bit matched / ignored masks; lanes t == 0 add the pair's non-ignored count to npig[k][a]
#include "common.h"
#include "kernels.h"
#include "eval_iou.h"

namespace sylph {

typedef unsigned long long u64;

// the wave's own writes (LDS or scratch) become visible to its other lanes
__device__ __forceinline__ void lvis_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// dynamic LDS: LVIS_MATCH_WAVES slices of detection boxes [D][4] f64 | IoU tile [D][G] f64 | state rows [G][64] bytes
__global__ __launch_bounds__(LVIS_MATCH_WAVES * 64) void lvis_match_kernel(
    const float* __restrict__ det, const int* __restrict__ det_off, const int* __restrict__ pair_cat, const int* __restrict__ pair_flags,
    const int* __restrict__ n_pairs, const double* __restrict__ gt_box, const double* __restrict__ gt_area, const int* __restrict__ gt_ignore,
    const int* __restrict__ gt_off, const double* __restrict__ iou_thr, int T, const double* __restrict__ area_rng, int A, int max_det,
    unsigned char* gt_scratch, u64* matched, u64* ignored, int* npig) {
  extern __shared__ double lvis_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long pl = (long)blockIdx.x * LVIS_MATCH_WAVES + wave;
  if (pl >= (long)*n_pairs) return;  // a surplus wave of the upper-bound grid
  const int p = (int)pl;
  const int d0 = det_off[p], nd = det_off[p + 1] - d0;
  const int g0 = gt_off[p], G = gt_off[p + 1] - g0;
  if (nd <= 0 && G <= 0) return;
  const int D = nd < max_det ? nd : max_det;  // nd <= max_det is the caller's contract; the slice holds max_det boxes at most
  double* dbox = lvis_lds + (size_t)wave * (LVIS_MATCH_SLICE_BYTES / 8);
  double* tile = dbox + (size_t)D * 4;
  const bool big = !lvis_match_fits(D, G);
  if (big && !gt_scratch) return;  // refused on the host (max_det, max_gt); counts beyond the caller's stated bounds touch nothing
  unsigned char* gs = big ? gt_scratch + (size_t)g0 * 64 : reinterpret_cast<unsigned char*>(tile + (size_t)D * G);
  const int kcat = pair_cat[p];
  const bool not_exhaustive = (pair_flags[p] & 1) != 0;

  for (int i = lane; i < D; i += 64) {
    const float* r = det + (size_t)(d0 + i) * 8;
    const double x0 = (double)r[1], y0 = (double)r[2], x1 = (double)r[3], y1 = (double)r[4];
    dbox[i * 4 + 0] = x0;
    dbox[i * 4 + 1] = y0;
    dbox[i * 4 + 2] = x1 - x0;
    dbox[i * 4 + 3] = y1 - y0;
  }
  for (int g = lane; g < G; g += 64) {
    const double ar = gt_area[g0 + g];
    const bool ig = gt_ignore[g0 + g] != 0;
    unsigned f = 0u;
    for (int a = 0; a < A; ++a)
      if (ig || ar < area_rng[2 * a] || ar > area_rng[2 * a + 1]) f |= 1u << a;
    u64* row = reinterpret_cast<u64*>(gs + (size_t)g * 64);
    for (int q = 0; q < 7; ++q) row[q] = 0ull;
    row[7] = (u64)f << 56;  // byte 63
  }
  lvis_wave_sync();
  if (!big) {
    const int cells = D * G;
    for (int idx = lane; idx < cells; idx += 64) {
      const int d = idx / G, g = idx - d * G;
      tile[idx] = coco_iou(dbox[d * 4], dbox[d * 4 + 1], dbox[d * 4 + 2], dbox[d * 4 + 3], gt_box + (size_t)(g0 + g) * 4, 0);
    }
  }
  lvis_wave_sync();

  const bool act = lane < A * T;
  const int a = act ? lane / T : 0, t = act ? lane - a * T : 0;
  const double thr0 = fmin(iou_thr[t], 1.0 - 1e-10);
  const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
  if (act && t == 0) {
    int cnt = 0;
    for (int g = 0; g < G; ++g) cnt += ((gs[(size_t)g * 64 + 63] >> a) & 1) ? 0 : 1;
    if (cnt) atomicAdd(&npig[kcat * A + a], cnt);
  }
  for (int d = 0; d < D; ++d) {
    int m = -1;
    bool dig = false;
    if (act) {
      const double dx = dbox[d * 4], dy = dbox[d * 4 + 1], dw = dbox[d * 4 + 2], dh = dbox[d * 4 + 3];
      double best = thr0;
      for (int pass = 0; pass < 2; ++pass) {  // non-ignored boxes first; the ignored ones only while nothing is matched
        if (pass == 1 && m >= 0) break;
        for (int g = 0; g < G; ++g) {
          const unsigned f = gs[(size_t)g * 64 + 63];
          if ((int)((f >> a) & 1u) != pass) continue;
          if (gs[(size_t)g * 64 + lane]) continue;  // matched at this (area, threshold) already
          const double iou = big ? coco_iou(dx, dy, dw, dh, gt_box + (size_t)(g0 + g) * 4, 0) : tile[(size_t)d * G + g];
          if (iou < best) continue;
          best = iou;  // an equal IoU replaces: the last of equal candidates wins
          m = g;
        }
      }
      if (m >= 0) {
        gs[(size_t)m * 64 + lane] = 1;  // a byte only this lane reads
        dig = (gs[(size_t)m * 64 + 63] >> a) & 1u;
      } else {
        const double da = dw * dh;
        dig = da < lo || da > hi || not_exhaustive;
      }
    }
    const u64 mm = __ballot(act && m >= 0), ii = __ballot(act && dig);
    if (lane == 0) {
      matched[d0 + d] = mm;
      ignored[d0 + d] = ii;
    }
  }
}

int launch_lvis_match(int max_pairs, const int* n_pairs, int K, const float* det, const int* det_off, const int* pair_cat, const int* pair_flags,
                      const double* gt_box, const double* gt_area, const int* gt_ignore, const int* gt_off, const double* iou_thr, int T,
                      const double* area_rng, int A, int max_det, unsigned char* gt_scratch, u64* matched, u64* ignored, int* npig,
                      hipStream_t s) {
  if (max_pairs <= 0 || K <= 0 || T <= 0 || A <= 0 || A > 4 || A * T > COCO_MATCH_LANES || max_det <= 0 || max_det > LVIS_MATCH_MAX_DETS)
    return (int)hipErrorInvalidValue;
  static_assert(LVIS_MATCH_MAX_DETS * 32 <= LVIS_MATCH_SLICE_BYTES, "the boxes of a pair's detections fit its wave's slice");
  constexpr int lds = LVIS_MATCH_WAVES * LVIS_MATCH_SLICE_BYTES;
  static PerDeviceOnce once;
  if (!once.run(current_device(), [] {
        return hipFuncSetAttribute((const void*)lvis_match_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds) == hipSuccess;
      }))
    return -7;
  if (hipMemsetAsync(npig, 0, (size_t)K * A * sizeof(int), s) != hipSuccess) return -8;
  const int blocks = (max_pairs + LVIS_MATCH_WAVES - 1) / LVIS_MATCH_WAVES;
  hipLaunchKernelGGL(lvis_match_kernel, dim3(blocks), dim3(LVIS_MATCH_WAVES * 64), lds, s, det, det_off, pair_cat, pair_flags, n_pairs, gt_box,
                     gt_area, gt_ignore, gt_off, iou_thr, T, area_rng, A, max_det, gt_scratch, matched, ignored, npig);
  return (int)hipGetLastError();
}

}  // namespace sylph
