// The box IoU of the evaluation kernels (coco_eval.hip, lvis_eval.hip): float64, in the operation order of tests/cocoeval_ref.py iou().
// Units that include this file are built without FMA contraction.
#pragma once
#include <hip/hip_runtime.h>

namespace sylph {

__device__ __forceinline__ double coco_iou(double dx, double dy, double dw, double dh, const double* __restrict__ g, int crowd) {
  const double gx = g[0], gy = g[1], gw = g[2], gh = g[3];
  const double iw = fmin(dx + dw, gx + gw) - fmax(dx, gx);
  const double ih = fmin(dy + dh, gy + gh) - fmax(dy, gy);
  if (iw <= 0.0 || ih <= 0.0) return 0.0;
  const double i = iw * ih;
  const double u = crowd ? dw * dh : dw * dh + gw * gh - i;
  return i / u;
}

}  // namespace sylph
