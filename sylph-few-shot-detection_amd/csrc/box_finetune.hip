// TFA-style fine-tuning of the FCOS box branch on the K shots, bf16: the layer behind the frozen bbox tower -- bbox_pred (4) + ctrness (1)
// [+ iou_overlap (1)], one 3x3 conv of Cout = 5 or 6 channels, and the per-level Scale -- under loss_fcos_loc / loss_fcos_ctr /
// loss_fcos_iou (fcos_outputs.py:675-741; the Meta-FCOS-pretrain-tfa-finetune yamls leave FREEZE_BBOX_BRANCH off).  These losses touch
// positive locations only, so the layer's input is cut out of the bbox tower ONCE per batch:
//
// box samples   box_assign_kernel  one thread per location of the padded pyramid: the claiming box (fcos_assign.h, the rule of
//                                  fcos_targets_kernel) and the positives of each 256-row block
//               box_scan_kernel    one block: exclusive scan of the block counts -> where each block's samples start, the total, the
//                                  overflow bit.  No atomic decides an order: sample p is the p-th positive in ascending row order.
//               box_emit_kernel    info (row, level, box, class) and targets (l, t, r, b) / stride, plain fp32 (fcos_outputs.py:185-189)
//               box_patch_kernel   patches[p][ky][kx][256] bf16 = bf16(relu(fma(x, a, b))) of the tower's last layer at the nine
//                                  neighbours -- gn_relu_pair of gn_stream.h, the operand values gn_taps_kernel multiplies -- zeros
//                                  outside the level's map
//
// box_grad_kernel, one pass over the bank.  Samples are cut into UNITS of BOX_GRAD_UNIT consecutive samples, a function of n alone; a
// block of six waves takes units.  k = (3 ky + kx) 256 + c indexes a patch and a row of the weights.
//   forward   a wave takes every sixth sample of the unit; a lane the channel pairs lane + 64 j:
//               z[n] = sum_k x[k] bf16(W[n][k]) + b[n]   fmaf chain per lane in ascending j, then the xor butterfly 32 .. 1: fixed order
//   loss      on lane-uniform values, plain fp32, with s = scales[level], tau = targets:
//               p = relu(s z[0:4]);  ious, gious of iou_loss.py:26-65;  ctr = compute_ctrness_targets (fcos_outputs.py:52-60)
//               loc = wgt (1 - giou), wgt = ctr with "ctrness" in BOX_QUALITY, else 1;  bce(z[4], ctr);  bce(z[5], iou or 0 below 0.3)
//               g[n] = d loss / d z[n]; channel 4 only with "ctrness", channel 5 only with "iou" (the reference detaches the other)
//   backward  thread t owns the channel pairs t + 384 j, j < 3: dW[n][k] += g[s][n] x[s][k] over the unit's samples in ascending s
//             (fmaf), 36 accumulators; db, d scales and the four sums by single threads in the same order
// The unit's partial (BOX_GRAD_PARTIAL floats) goes to the workspace; the ordered tree of partial_sum.h (fan-in 64) adds the partials and
// its sink here, BoxGradSink, writes torch's (Cout, 256, 3, 3) layout: no atomics, the same bits on every grid.
// The products run on the VALU: Cout is 5 or 6, so an MFMA tile would be 10 / 16 zeros, and the whole bank (a few thousand rows of
// 4.6 KB) is read twice per step, from L2 / MALL the second time.
#include <stdlib.h>

#include "fcos_assign.h"
#include "gn_stream.h"
#include "kernels.h"
#include "partial_sum.h"

namespace sylph {

// ---- samples ------------------------------------------------------------------------------------------------------------------------

// grid (gx, nseg): block (bx, seg) owns map-relative rows [256 bx, 256 bx + 256) of segment seg; blk_cnt[seg * gx + bx] = its positives
__global__ __launch_bounds__(256) void box_assign_kernel(const SegDesc* __restrict__ segs, int nlevels, FcosTargetCfg cfg, int n_gt,
                                                         const float* __restrict__ boxes, const int* __restrict__ gt_image,
                                                         int* __restrict__ assign, int* __restrict__ blk_cnt) {
  const int seg = blockIdx.y, b = seg / nlevels, lv = seg - b * nlevels;
  const SegDesc& sd = segs[seg];
  const int W = sd.out_W, n = sd.out_H * W, stride = cfg.strides[lv];
  const int i = blockIdx.x * 256 + threadIdx.x;
  int k = -1;
  if (blockIdx.x * 256 < n) {  // block-uniform
    if (i < n) {
      const FcosSegCtx sc = fcos_seg_ctx(cfg, b, lv, n_gt, boxes, gt_image);
      const int yi = i / W, xi = i - yi * W;
      k = fcos_assign(cfg, sc, b, n_gt, boxes, gt_image, (float)(xi * stride + stride / 2), (float)(yi * stride + stride / 2));
      assign[sd.out_row0 + i] = k;
    }
  }
  const int cnt = __syncthreads_count(k >= 0);
  if (threadIdx.x == 0) blk_cnt[seg * gridDim.x + blockIdx.x] = cnt;
}

// one block: blk_cnt -> its exclusive scan in place; count_out = the total; status = 1 when the total exceeds max_samples
__global__ __launch_bounds__(256) void box_scan_kernel(int* __restrict__ blk_cnt, int nblk, int max_samples, int* __restrict__ count_out,
                                                       int* __restrict__ status) {
  __shared__ int part[256];
  const int t = threadIdx.x, per = (nblk + 255) / 256, i0 = t * per, i1 = min(nblk, i0 + per);
  int s = 0;
  for (int i = i0; i < i1; ++i) s += blk_cnt[i];
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    int run = 0;
    for (int i = 0; i < 256; ++i) { const int v = part[i]; part[i] = run; run += v; }
    *count_out = run;
    *status = run > max_samples ? 1 : 0;
  }
  __syncthreads();
  int run = part[t];
  for (int i = i0; i < i1; ++i) { const int v = blk_cnt[i]; blk_cnt[i] = run; run += v; }
}

__global__ __launch_bounds__(256) void box_emit_kernel(const SegDesc* __restrict__ segs, int nlevels, FcosTargetCfg cfg,
                                                       const float* __restrict__ boxes, const int* __restrict__ gt_class,
                                                       const int* __restrict__ assign, const int* __restrict__ blk_off, int max_samples,
                                                       int* __restrict__ info, float* __restrict__ targets) {
  __shared__ int wcnt[4];
  const int seg = blockIdx.y, lv = seg % nlevels;
  const SegDesc& sd = segs[seg];
  const int W = sd.out_W, n = sd.out_H * W, stride = cfg.strides[lv];
  if (blockIdx.x * 256 >= n) return;  // block-uniform
  const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k = i < n ? assign[sd.out_row0 + i] : -1;
  const unsigned long long m = __ballot(k >= 0);
  if (lane == 0) wcnt[wave] = __popcll(m);
  __syncthreads();
  int p = blk_off[seg * gridDim.x + blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) p += wcnt[w];
  if (k < 0 || p >= max_samples) return;
  const int yi = i / W, xi = i - yi * W;
  const float x = (float)(xi * stride + stride / 2), y = (float)(yi * stride + stride / 2), fs = (float)stride;
  const float x0 = boxes[4 * k], y0 = boxes[4 * k + 1], x1 = boxes[4 * k + 2], y1 = boxes[4 * k + 3];
  *reinterpret_cast<int4*>(info + 4 * (size_t)p) = make_int4(sd.out_row0 + i, lv, k, gt_class[k]);
  *reinterpret_cast<float4*>(targets + 4 * (size_t)p) = make_float4((x - x0) / fs, (y - y0) / fs, (x1 - x) / fs, (y1 - y) / fs);
}

// block of 288 threads per sample: thread (tap = tid / 32, 8 channels 8 (tid % 32) ..)
__global__ __launch_bounds__(288) void box_patch_kernel(const bf16_t* __restrict__ x, const float2* __restrict__ coef,
                                                        const SegDesc* __restrict__ segs, int nlevels, int rows_per_image,
                                                        const int* __restrict__ info, const int* __restrict__ count, int max_samples,
                                                        bf16_t* __restrict__ patches) {
  const int n = min(*count, max_samples);
  const int tap = threadIdx.x >> 5, c8 = (threadIdx.x & 31) * 8, ky = tap / 3, kx = tap - 3 * ky;
  for (int p = blockIdx.x; p < n; p += gridDim.x) {
    const int row = info[4 * (size_t)p], lv = info[4 * (size_t)p + 1];
    const int seg = (row / rows_per_image) * nlevels + lv;
    const SegDesc& sd = segs[seg];
    const int i = row - sd.out_row0, yi = i / sd.out_W, xi = i - yi * sd.out_W;
    const int yy = yi + ky - 1, xx = xi + kx - 1;
    u32x4 v = {0u, 0u, 0u, 0u};
    if ((unsigned)yy < (unsigned)sd.out_H && (unsigned)xx < (unsigned)sd.out_W) {
      const u32x4 raw = *reinterpret_cast<const u32x4*>(x + ((size_t)sd.out_row0 + (size_t)yy * sd.out_W + xx) * 256 + c8);
      const float2* cp = coef + (size_t)seg * 256 + c8;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float2 q0 = cp[2 * e], q1 = cp[2 * e + 1];
        v[e] = gn_relu_pair(raw[e], f32x2{q0.x, q1.x}, f32x2{q0.y, q1.y});
      }
    }
    *reinterpret_cast<u32x4*>(patches + (size_t)p * 2304 + tap * 256 + c8) = v;
  }
}

int launch_box_samples(const void* x, const float2* coef, const SegDesc* segs, int nseg, int nlevels, int max_rows, int rows_per_image,
                       const FcosTargetCfg& cfg, int n_gt, const float* boxes, const int* gt_class, const int* gt_image, int* assign, int* blk,
                       int max_samples, void* patches, float* targets, int* info, int* count, int* status, hipStream_t s) {
  if (nseg <= 0 || nlevels <= 0 || nlevels > 8 || nseg % nlevels != 0 || max_rows <= 0 || max_samples < 0) return -1;
  const int gx = box_samples_gx(max_rows);
  hipLaunchKernelGGL(box_assign_kernel, dim3(gx, nseg), dim3(256), 0, s, segs, nlevels, cfg, n_gt, boxes, gt_image, assign, blk);
  hipLaunchKernelGGL(box_scan_kernel, dim3(1), dim3(256), 0, s, blk, gx * nseg, max_samples, count, status);
  if (max_samples > 0) {
    hipLaunchKernelGGL(box_emit_kernel, dim3(gx, nseg), dim3(256), 0, s, segs, nlevels, cfg, boxes, gt_class, assign, blk, max_samples, info,
                       targets);
    hipLaunchKernelGGL(box_patch_kernel, dim3(max_samples < 8192 ? max_samples : 8192), dim3(288), 0, s, (const bf16_t*)x, coef, segs, nlevels,
                       rows_per_image, info, count, max_samples, (bf16_t*)patches);
  }
  return (int)hipGetLastError();
}

// ---- loss and gradient ----------------------------------------------------------------------------------------------------------------

// BCE with logits and its derivative: loss = max(z, 0) - z t + log1p(exp(-|z|)), g = sigmoid(z) - t
__device__ __forceinline__ void bce_one(float z, float t, float& loss, float& g) {
  const float e = expf(-fabsf(z));
  const float inv = 1.f / (1.f + e);
  loss = fmaxf(z, 0.f) - z * t + log1pf(e);
  g = (z >= 0.f ? inv : e * inv) - t;
}

struct BoxLoss { float g[6], gscale, sums[4]; };

// one sample; quality: bit 0 "ctrness", bit 1 "iou"
__device__ __forceinline__ BoxLoss box_loss_one(const float* z, int cout, float s, float4 tau, int quality, int iou_mask) {
  BoxLoss o;
  const float tg[4] = {tau.x, tau.y, tau.z, tau.w};
  float u[4], p[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { u[i] = s * z[i]; p[i] = fmaxf(u[i], 0.f); }
  const float ta = (tg[0] + tg[2]) * (tg[1] + tg[3]);
  const float pw = p[0] + p[2], ph = p[1] + p[3], pa = pw * ph;
  const float wi = fminf(p[0], tg[0]) + fminf(p[2], tg[2]), hi = fminf(p[3], tg[3]) + fminf(p[1], tg[1]);
  const float gw = fmaxf(p[0], tg[0]) + fmaxf(p[2], tg[2]), gh = fmaxf(p[3], tg[3]) + fmaxf(p[1], tg[1]);
  const float ac = gw * gh, ai = wi * hi, au = ta + pa - ai;
  const float A = ai + 1.f, U = au + 1.f;
  const float iou = A / U, giou = iou - (ac - au) / ac;
  const float lr0 = fminf(tg[0], tg[2]) / fmaxf(tg[0], tg[2]), tb0 = fminf(tg[1], tg[3]) / fmaxf(tg[1], tg[3]);
  const float ctr = sqrtf(lr0 * tb0);
  const float wgt = (quality & 1) ? ctr : 1.f;
  o.sums[0] = wgt * (1.f - giou);
  o.sums[3] = ctr;
  // d giou / d p_i = (dai U - A dau) / U^2 + (dau ac - au dac) / ac^2, dau = dpa - dai
  const float U2 = U * U, ac2 = ac * ac;
  o.gscale = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bool horiz = (i & 1) == 0;  // left, right
    const float dpa = horiz ? ph : pw;
    const float dai = p[i] < tg[i] ? (horiz ? hi : wi) : 0.f;
    const float dac = p[i] > tg[i] ? (horiz ? gh : gw) : 0.f;
    const float dau = dpa - dai;
    const float dg = (dai * U - A * dau) / U2 + (dau * ac - au * dac) / ac2;
    const float gp = u[i] > 0.f ? -(wgt * dg) : 0.f;  // d loc / d (s z_i)
    o.g[i] = gp * s;
    o.gscale += gp * z[i];
  }
  float l4, g4;
  bce_one(z[4], ctr, l4, g4);
  o.sums[1] = l4;
  o.g[4] = (quality & 1) ? g4 : 0.f;
  o.sums[2] = 0.f;
  o.g[5] = 0.f;
  if (cout > 5) {
    const float it = (iou_mask && iou < 0.3f) ? 0.f : iou;
    float l5, g5;
    bce_one(z[5], it, l5, g5);
    o.sums[2] = l5;
    o.g[5] = (quality & 2) ? g5 : 0.f;
  }
  return o;
}

constexpr int BG_K = 2304, BG_PAIRS = BG_K / 2;

__global__ __launch_bounds__(384) void box_grad_kernel(int n, const bf16_t* __restrict__ patches, const float* __restrict__ targets,
                                                       const int* __restrict__ info, const float* __restrict__ w, const float* __restrict__ bias,
                                                       const float* __restrict__ scales, int cout, int nlevels, int quality, int iou_mask,
                                                       float* __restrict__ part, float* __restrict__ z_out, float* __restrict__ g_out) {
  __shared__ unsigned wl[6][BG_PAIRS];          // bf16(W) as channel pairs, k order of the patches; rows >= cout zero
  __shared__ float gs[BOX_GRAD_UNIT][8];        // g[0:6] | d loss / d scale | level
  __shared__ float ls[BOX_GRAD_UNIT][4];        // the sample's four sums
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < 6 * BG_PAIRS; i += 384) {
    const int c = i / BG_PAIRS, pr = i - c * BG_PAIRS, tap = pr >> 7, ci = (pr & 127) * 2;
    bf16x2 q = {(bf16_t)0.f, (bf16_t)0.f};
    if (c < cout) {
      q[0] = (bf16_t)w[w3x3_torch(c, tap, ci)];
      q[1] = (bf16_t)w[w3x3_torch(c, tap, ci + 1)];
    }
    wl[c][pr] = __builtin_bit_cast(unsigned, q);
  }
  __syncthreads();
  const int n_units = (n + BOX_GRAD_UNIT - 1) / BOX_GRAD_UNIT;
  for (int unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
    const int s0 = unit * BOX_GRAD_UNIT, ns = min(BOX_GRAD_UNIT, n - s0);
    // forward + loss
    for (int s = wave; s < BOX_GRAD_UNIT; s += 6) {
      if (s >= ns) {  // wave-uniform: a sample past the bank contributes zeros
        if (lane < 8) gs[s][lane] = 0.f;
        if (lane < 4) ls[s][lane] = 0.f;
        continue;
      }
      const unsigned* xp = reinterpret_cast<const unsigned*>(patches + (size_t)(s0 + s) * BG_K);
      float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < BG_PAIRS / 64; ++j) {
        const unsigned xv = xp[lane + 64 * j];
        const float x0 = __uint_as_float(xv << 16), x1 = __uint_as_float(xv & 0xffff0000u);
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          const unsigned wv = wl[c][lane + 64 * j];
          acc[c] = fmaf(x0, __uint_as_float(wv << 16), acc[c]);
          acc[c] = fmaf(x1, __uint_as_float(wv & 0xffff0000u), acc[c]);
        }
      }
#pragma unroll
      for (int c = 0; c < 6; ++c)
        for (int o = 32; o > 0; o >>= 1) acc[c] += __shfl_xor(acc[c], o);
      float z[6];
#pragma unroll
      for (int c = 0; c < 6; ++c) z[c] = c < cout ? acc[c] + bias[c] : 0.f;
      const int lv = min(max(info[4 * (size_t)(s0 + s) + 1], 0), nlevels - 1);
      const float4 tau = *reinterpret_cast<const float4*>(targets + 4 * (size_t)(s0 + s));
      const BoxLoss o = box_loss_one(z, cout, scales[lv], tau, quality, iou_mask);
      if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 6; ++c) gs[s][c] = o.g[c];
        gs[s][6] = o.gscale;
        gs[s][7] = (float)lv;
#pragma unroll
        for (int q = 0; q < 4; ++q) ls[s][q] = o.sums[q];
      }
#pragma unroll
      for (int c = 0; c < 6; ++c)  // (lane c writes channel c: a register array is never indexed by the lane)
        if (lane == c && c < cout) {
          if (z_out) z_out[(size_t)(s0 + s) * cout + c] = z[c];
          if (g_out) g_out[(size_t)(s0 + s) * cout + c] = o.g[c];
        }
    }
    __syncthreads();
    // backward: dW[c][k] of the unit
    float dw[3][6][2];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int c = 0; c < 6; ++c) dw[j][c][0] = dw[j][c][1] = 0.f;
    for (int s = 0; s < ns; ++s) {
      const unsigned* xp = reinterpret_cast<const unsigned*>(patches + (size_t)(s0 + s) * BG_K);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const unsigned xv = xp[tid + 384 * j];
        const float x0 = __uint_as_float(xv << 16), x1 = __uint_as_float(xv & 0xffff0000u);
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          const float g = gs[s][c];
          dw[j][c][0] = fmaf(g, x0, dw[j][c][0]);
          dw[j][c][1] = fmaf(g, x1, dw[j][c][1]);
        }
      }
    }
    float* pp = part + (size_t)unit * BOX_GRAD_PARTIAL;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int c = 0; c < 6; ++c)
        *reinterpret_cast<float2*>(pp + c * BG_K + 2 * (tid + 384 * j)) = make_float2(dw[j][c][0], dw[j][c][1]);
    if (tid < 6) {  // db
      float a = 0.f;
      for (int s = 0; s < ns; ++s) a += gs[s][tid];
      pp[BOX_GRAD_DB + tid] = a;
    } else if (tid >= 64 && tid < 72) {  // d scales
      const int lv = tid - 64;
      float a = 0.f;
      for (int s = 0; s < ns; ++s) a += (int)gs[s][7] == lv ? gs[s][6] : 0.f;
      pp[BOX_GRAD_DS + lv] = a;
    } else if (tid >= 128 && tid < 132) {  // the sums
      float a = 0.f;
      for (int s = 0; s < ns; ++s) a += ls[s][tid - 128];
      pp[BOX_GRAD_SUMS + tid - 128] = a;
    }
    __syncthreads();  // gs / ls are rewritten by the next unit
  }
}

// the sink of the tree's final kernel: element i of the summed partial -> grad_w (cout, 256, 3, 3), grad_b (cout), grad_scales (nlevels),
// sums (4).  An empty bank (no partial) sums to zeros
struct BoxGradSink {
  int cout, nlevels;
  float *grad_w, *grad_b, *grad_scales, *sums;
  __device__ void operator()(int i, float s) const {
    if (i < 6 * BG_K) {
      const int c = i / BG_K, k = i - c * BG_K, tap = k >> 8, ci = k & 255;
      if (c < cout) grad_w[w3x3_torch(c, tap, ci)] = s;
    } else if (i >= BOX_GRAD_DB && i < BOX_GRAD_DB + 6) {
      if (i - BOX_GRAD_DB < cout) grad_b[i - BOX_GRAD_DB] = s;
    } else if (i >= BOX_GRAD_DS && i < BOX_GRAD_DS + 8) {
      if (i - BOX_GRAD_DS < nlevels) grad_scales[i - BOX_GRAD_DS] = s;
    } else if (i >= BOX_GRAD_SUMS) {
      sums[i - BOX_GRAD_SUMS] = s;
    }
  }
};

int box_grad_units(int n) { return (n + BOX_GRAD_UNIT - 1) / BOX_GRAD_UNIT; }

size_t box_grad_ws_floats(int n) { return partial_tree(box_grad_units(n), BOX_GRAD_FANIN).planes * BOX_GRAD_PARTIAL; }

int launch_box_grad(int n, const void* patches, const float* targets, const int* info, const float* w, const float* bias, const float* scales,
                    int cout, int nlevels, int quality, int iou_mask, float* ws, float* sums, float* grad_w, float* grad_b, float* grad_scales,
                    float* z_out, float* g_out, hipStream_t s) {
  if (n < 0 || cout < 5 || cout > 6 || nlevels < 1 || nlevels > 8 || (n > 0 && !ws)) return -1;
  const int u = box_grad_units(n);
  if (u > 0) {
    // SYLPH_BOX_GRAD_BLOCKS: another block cap (tests: a block then takes several units; the results must keep their bits)
    const int cap = block_cap("SYLPH_BOX_GRAD_BLOCKS", BOX_GRAD_MAX_BLOCKS);
    hipLaunchKernelGGL(box_grad_kernel, dim3(u < cap ? u : cap), dim3(384), 0, s, n, (const bf16_t*)patches, targets, info, w, bias, scales, cout,
                       nlevels, quality, iou_mask, ws, z_out, g_out);
  }
  partial_final(partial_sum_passes(ws, u, BOX_GRAD_PARTIAL, BOX_GRAD_FANIN, s), BOX_GRAD_PARTIAL, BOX_GRAD_SUMS + 4,
                BoxGradSink{cout, nlevels, grad_w, grad_b, grad_scales, sums}, s);
  return (int)hipGetLastError();
}

}  // namespace sylph
