// The ordered partial-sum tree behind every training gradient (finetune.hip, box_finetune.hip, codegen_train.hip).  No atomics: a
// gradient kernel cuts its work into UNITS -- a function of the problem, never of the grid -- and writes one partial of `plane` floats per
// unit.  A pass adds `fanin` consecutive partials into one, in ascending order; passes repeat until at most `fanin` are left, and a final
// kernel adds those in order and hands every sum to the path's SINK, which scatters it into torch's layout.  The same inputs therefore
// give the same bits on every grid.  The workspace holds the levels back to back: level 0 (the units' partials) at ws, level l + 1 right
// behind the n_l planes of level l.
//
// Header-only, as nms_walk.h is: the build has no relocatable device code, so each translation unit instantiates its own copy of the
// kernels (the sum kernel has internal linkage; the final kernel is a template over the unit's own sink type).
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>

namespace sylph {

// the grid cap of a gradient kernel: the environment's positive value (tests: a block then takes several units; the bits must not
// move), else the default
inline int block_cap(const char* env_name, int dflt) {
  const char* e = getenv(env_name);
  return e && atoi(e) > 0 ? atoi(e) : dflt;
}

// planes: the partials of every level together (what the workspace holds); passes: the launches, the final one included
struct PartialTree { size_t planes; int passes; };
inline PartialTree partial_tree(int units, int fanin) {
  PartialTree t{(size_t)units, 1};
  for (int n = units; n > fanin; ++t.passes) { n = (n + fanin - 1) / fanin; t.planes += (size_t)n; }
  return t;
}

// out[c][i] = sum of in[fanin c + k][i], k = 0 .. fanin - 1 (those below n_in), in that order; grid (ceil(plane / 256), chunks)
static __global__ __launch_bounds__(256) void partial_sum_kernel(const float* __restrict__ in, int n_in, int plane, int fanin,
                                                                 float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
  if (i >= plane) return;
  const int k1 = min(n_in, fanin * (c + 1));
  float s = 0.f;
  for (int k = fanin * c; k < k1; ++k) s += in[(size_t)k * plane + i];
  out[(size_t)c * plane + i] = s;
}

// the last n_in <= fanin partials summed in order; element i < count of the sum goes to sink(i, s).  n_in = 0: every sum is zero
template <class Sink>
__global__ __launch_bounds__(256) void partial_final_kernel(const float* __restrict__ in, int n_in, int plane, int count, Sink sink) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  float s = 0.f;
  for (int k = 0; k < n_in; ++k) s += in[(size_t)k * plane + i];
  sink(i, s);
}

// runs the passes over the `units` partials at ws; returns the last level: where it starts and the n <= fanin partials it holds
struct PartialLevel { const float* in; int n; };
inline PartialLevel partial_sum_passes(float* ws, int units, int plane, int fanin, hipStream_t s) {
  float* in = ws;
  int n = units;
  while (n > fanin) {
    const int m = (n + fanin - 1) / fanin;
    float* out = in + (size_t)n * plane;
    hipLaunchKernelGGL(partial_sum_kernel, dim3((plane + 255) / 256, m), dim3(256), 0, s, in, n, plane, fanin, out);
    in = out;
    n = m;
  }
  return {in, n};
}

// the final kernel over the first `count` floats of the last level's planes
template <class Sink>
inline void partial_final(PartialLevel last, int plane, int count, const Sink& sink, hipStream_t s) {
  hipLaunchKernelGGL(partial_final_kernel<Sink>, dim3((count + 255) / 256), dim3(256), 0, s, last.in, last.n, plane, count, sink);
}

}  // namespace sylph
