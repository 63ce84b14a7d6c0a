// FCOSOutputs.compute_targets_for_locations + get_sample_region (fcos_outputs.py:193-349) for ONE location: which ground-truth box claims
// it.  Shared by fcos_targets_kernel (finetune.hip: the box's class is the label) and box_assign_kernel (box_finetune.hip: the box is the
// regression target).  Plain fp32, comparison by comparison as the reference: both units are compiled without FMA contraction.
// Device code only.
#pragma once
#include "kernels.h"

namespace sylph {

constexpr float FCOS_INF = 100000000.f;  // fcos_outputs.py:27

// what a segment (image b, level lv) needs of the batch's boxes before its locations are walked
struct FcosSegCtx {
  int first;          // index of image b's first box (n_gt: none)
  bool region_empty;  // "no gt" of get_sample_region: the centre-x of the image's FIRST box is 0 (fcos_outputs.py:227)
  float lo, hi, st;   // the level's range of the largest regression target; `strides[level] * radius`
};

__device__ __forceinline__ FcosSegCtx fcos_seg_ctx(const FcosTargetCfg& cfg, int b, int lv, int n_gt, const float* __restrict__ boxes,
                                                   const int* __restrict__ gt_image) {
  FcosSegCtx s;
  s.lo = cfg.lo[lv]; s.hi = cfg.hi[lv];
  s.st = (float)((double)cfg.strides[lv] * (double)cfg.radius);  // a Python float, cast by the tensor op
  int first = 0;
  while (first < n_gt && gt_image[first] != b) ++first;
  s.first = first;
  s.region_empty = cfg.center_sample && first < n_gt && (boxes[4 * first] + boxes[4 * first + 2]) * 0.5f == 0.f;
  return s;
}

// the box of image b that claims location (x, y): the smallest area, the lowest index among equals; -1: background
__device__ __forceinline__ int fcos_assign(const FcosTargetCfg& cfg, const FcosSegCtx& sc, int b, int n_gt, const float* __restrict__ boxes,
                                           const int* __restrict__ gt_image, float x, float y) {
  float best = FCOS_INF;
  int hit = -1;
  for (int k = sc.first; k < n_gt; ++k) {
    if (gt_image[k] != b) continue;
    const float x0 = boxes[4 * k], y0 = boxes[4 * k + 1], x1 = boxes[4 * k + 2], y1 = boxes[4 * k + 3];
    const float l = x - x0, t = y - y0, r = x1 - x, bt = y1 - y;
    bool inside;
    if (cfg.center_sample) {
      const float cx = (x0 + x1) * 0.5f, cy = (y0 + y1) * 0.5f;
      const float xmin = cx - sc.st, ymin = cy - sc.st, xmax = cx + sc.st, ymax = cy + sc.st;
      const float c0 = xmin > x0 ? xmin : x0, c1 = ymin > y0 ? ymin : y0, c2 = xmax > x1 ? x1 : xmax, c3 = ymax > y1 ? y1 : ymax;
      inside = !sc.region_empty && fminf(fminf(x - c0, y - c1), fminf(c2 - x, c3 - y)) > 0.f;
    } else {
      inside = fminf(fminf(l, t), fminf(r, bt)) > 0.f;
    }
    const float m = fmaxf(fmaxf(l, t), fmaxf(r, bt));
    const float area = (x1 - x0) * (y1 - y0);
    if (inside && m >= sc.lo && m <= sc.hi && area < best) { best = area; hit = k; }
  }
  return hit;
}

}  // namespace sylph
