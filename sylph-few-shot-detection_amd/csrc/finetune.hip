// TFA-style fine-tuning of the class-conditional layer on stored tower outputs, bf16: FCOS classification targets, and loss + gradient of
// the sigmoid focal loss with respect to the class codes (CondConvBasic / cls_logits: N x 256 weights + N biases).  Everything in front
// of that layer is frozen (configs/COCO-Detection/TFA/FCOS_finetune.yaml: FREEZE_CLS_TOWER, FREEZE_BBOX_TOWER), so one gradient step is one
// streaming pass over the cls tower's raw output -- the tensor gn_logits_kernel scores -- plus an outer product.
//
// fcos_targets_kernel   FCOSOutputs.compute_targets_for_locations + get_sample_region (fcos_outputs.py:193-349), labels only: one thread
//                       per location of the padded pyramid, a loop over the image's boxes in plain fp32 (compiled without FMA
//                       contraction: every comparison is the reference's).
//
// cls_grad_kernel       for one block of up to 32 classes (class n0 + n is column n):
//                         z[p][n]  = sum_c xn[p][c] bf16(W[n][c]) + b[n],   xn = bf16(relu(fma(x, a, b)))  (gn_stream.h: gn_logits_kernel's operand)
//                         loss     = sum_(p, n) focal(z, t),  t[p][n] = (label[p] == n0 + n)     (fvcore sigmoid_focal_loss, unnormalised)
//                         g        = d loss / d z
//                         dW[n][c] = sum_p g[p][n] xn[p][c],   db[n] = sum_p g[p][n]
//   A wave takes 32-row groups.  Forward: positions are the MFMA rows, classes the columns (A = xn, B = codes), so a lane holds ONE class
//   (column l31) and 16 positions (row (r & 3) + 8 (r >> 2) + 4 lh in register r), and the 32 x 32 tile g is, as it stands in the
//   registers, the B operand of dW^T = xn^T g: registers 8 s .. 8 s + 7 are k-step s, element j of lane half lh being position
//   16 s + 8 (j >> 2) + 4 lh + (j & 3).  g enters as a bf16 hi + lo pair, two MFMAs into the same accumulator: the gradients carry 16
//   mantissa bits of g, not 8.  Only xn needs a transpose.  While the forward runs, every lane leaves its normalised 16-byte pieces in
//   a wave-private LDS image of the group, [2 halves of 128 channels][32 rows][256 B], chunk ch of row r at 256 r + 16 (ch ^ sw(r)),
//   sw(r) = ((r & 3) << 2) | ((r >> 2) & 3); ds_read_b64_tr_b16 reads it back column-major: per 16-lane group a block of 4 positions x 16
//   channels, lane i receiving channel i of the four positions -- for the lane group (lh, 16-channel half) and the block (k-step s, j >> 2)
//   exactly the permuted k order above.  The reads run with EXEC all ones: every branch around them is wave-uniform, rows past a map are
//   clamped and computed (g = 0), never masked.  Same-wave LDS traffic is ordered: no barrier in the loop.
//   No atomics.  The row groups are cut into UNITS of CLS_GRAD_UNIT_GROUPS consecutive groups -- a function of the tile table alone, not of
//   the grid -- and a wave keeps the 8 x 16 accumulator registers of dW^T, db and the loss over one unit, then writes the unit's partial
//   ([256][32] dW^T | [32] db | loss, CLS_GRAD_PARTIAL floats).  The ordered tree of partial_sum.h (fan-in 64) adds the partials; its
//   sink here, ClsGradSink, writes the N x 256 layout: the same inputs give the same bits whatever grid runs them.
//   Compiler's resource report (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): cls_grad_kernel 256 VGPRs + 170 AGPRs, 0 bytes
//   of scratch, 22 SGPRs spilled to VGPR lanes, 90 624 bytes of LDS, occupancy 1 wave per SIMD (one block per CU).  The AGPRs are spill
//   space: hipcc computes the dW^T tiles in VGPRs and copies them to AGPRs and back (~650 v_accvgpr moves in the kernel, most of them in
//   the row-group loop).  fcos_targets_kernel: 15 VGPRs, no scratch.
//   Measured (tools/bench_finetune.py, profiles/finetune_bench.txt): N = 20 on a record of 100 images of 800 x 1344, 0.59 ms against
//   0.30 ms of gn_logits_kernel on the same record; the loop is VALU-bound (focal loss, GroupNorm, AGPR copies), not HBM-bound.
#include <stdlib.h>

#include "fcos_assign.h"
#include "gn_stream.h"
#include "kernels.h"
#include "partial_sum.h"

namespace sylph {

// segs: the head's (image, level) segments, image-major; gt_*: the boxes of the whole batch; lo / hi of a level from sizes_of_interest:
// [-1, s0], [s0, s1], .., [s_last, INF]
__global__ __launch_bounds__(256) void fcos_targets_kernel(const SegDesc* __restrict__ segs, int nlevels, FcosTargetCfg cfg, int n_gt,
                                                           const float* __restrict__ boxes, const int* __restrict__ gt_class,
                                                           const int* __restrict__ gt_image, int* __restrict__ labels,
                                                           int* __restrict__ num_pos) {
  const int seg = blockIdx.y, b = seg / nlevels, lv = seg - b * nlevels;
  const SegDesc& sd = segs[seg];
  const int W = sd.out_W, n = sd.out_H * W, stride = cfg.strides[lv];
  const FcosSegCtx sc = fcos_seg_ctx(cfg, b, lv, n_gt, boxes, gt_image);
  int pos = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int yi = i / W, xi = i - yi * W;
    const float x = (float)(xi * stride + stride / 2), y = (float)(yi * stride + stride / 2);
    const int k = fcos_assign(cfg, sc, b, n_gt, boxes, gt_image, x, y);
    const int lab = k >= 0 ? gt_class[k] : -1;
    labels[sd.out_row0 + i] = lab;
    pos += lab >= 0;
  }
  // positives: an integer count (exact in any order)
  for (int o = 32; o > 0; o >>= 1) pos += __shfl_xor(pos, o);
  if ((threadIdx.x & 63) == 0 && pos) atomicAdd(num_pos, pos);
}

int launch_fcos_targets(const SegDesc* segs, int nseg, int nlevels, int max_rows, const FcosTargetCfg& cfg, int n_gt, const float* boxes,
                        const int* gt_class, const int* gt_image, int* labels, int* num_pos, hipStream_t s) {
  if (nseg <= 0 || nlevels <= 0 || nlevels > 8 || nseg % nlevels != 0 || max_rows <= 0) return -1;
  if (hipMemsetAsync(num_pos, 0, sizeof(int), s) != hipSuccess) return -2;
  const int gx = (max_rows + 255) / 256;
  hipLaunchKernelGGL(fcos_targets_kernel, dim3(gx < 64 ? gx : 64, nseg), dim3(256), 0, s, segs, nlevels, cfg, n_gt, boxes, gt_class, gt_image,
                     labels, num_pos);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_ptr;

constexpr int CG_W_PITCH = 528;  // bytes per code row in LDS

// byte offset of 16-byte chunk gc (8 channels: 0 .. 31) of row r in a wave's image
__device__ __forceinline__ int xt_off(int r, int gc) {
  return 8192 * (gc >> 4) + 256 * r + 16 * ((gc & 15) ^ (((r & 3) << 2) | ((r >> 2) & 3)));
}

// focal loss and d loss / d z of one logit: fvcore.nn.sigmoid_focal_loss restated on u = (2 t - 1) z, p_t = sigmoid(u):
//   ce = -log p_t = max(-u, 0) + log1p(exp(-|u|)),  loss = a_t (1 - p_t)^gamma ce,  g = a_t (2 t - 1) (1 - p_t)^gamma (-gamma p_t ce - (1 - p_t))
// On the hardware's exp2 / log2 / rcp (1 ulp each): the library expf / log1pf / division made this function 330 VALU instructions per
// logit and the kernel VALU-bound at 2.8 x the scoring launch.  log1p(e), 0 < e <= 1, as log(w) e / (w - 1) with w = fl(1 + e): w - 1 is
// exact, and the quotient undoes the rounding of 1 + e, so ce keeps its relative accuracy where e is tiny (w == 1: log1p(e) = e).
__device__ __forceinline__ void focal_one(float z, bool t, float alpha, float gamma, float& loss, float& g) {
  const float u = t ? z : -z;
  const float e = __builtin_amdgcn_exp2f(fabsf(u) * -1.4426950408889634f);
  const float w = 1.f + e;
  const float inv = __builtin_amdgcn_rcpf(w);
  const float pt = u >= 0.f ? inv : e * inv, q = u >= 0.f ? e * inv : inv;
  const float d = w - 1.f;
  const float l1p = d == 0.f ? e : (__builtin_amdgcn_logf(w) * 0.6931471805599453f) * (e * __builtin_amdgcn_rcpf(d));
  const float ce = fmaxf(-u, 0.f) + l1p;
  const float mod = gamma == 2.f ? q * q : (gamma == 0.f ? 1.f : powf(q, gamma));
  const float at = alpha >= 0.f ? (t ? alpha : 1.f - alpha) : 1.f;
  const float am = at * mod;
  loss = am * ce;
  const float gs = am * (-gamma * pt * ce - q);
  g = t ? gs : -gs;
}

// x: raw tower output [rows][ld] bf16; coef: [segments][256] (a, b); w: [32][256] bf16, rows >= nb zero; bias: [32] fp32 (zeros without a
// bias); labels: [rows] class index or -1; n0: class index of column 0; part: [units][CLS_GRAD_PARTIAL]
__global__ __launch_bounds__(256) void cls_grad_kernel(const bf16_t* __restrict__ x, int ld, const float2* __restrict__ coef,
                                                       const bf16_t* __restrict__ w, const float* __restrict__ bias, int nb, int n0,
                                                       const int* __restrict__ labels, float alpha, float gamma,
                                                       float* __restrict__ part, const SegDesc* __restrict__ segs,
                                                       const int2* __restrict__ tiles, int n_tiles) {
  __shared__ __attribute__((aligned(16))) float cf[4][512];               // per wave: (a0, a1, b0, b1) per channel pair of its current segment
  __shared__ __attribute__((aligned(16))) unsigned char xt[4][16384];     // per wave: the normalised group, see above
  __shared__ __attribute__((aligned(16))) unsigned char wl[32 * CG_W_PITCH];  // the block's codes
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;

  // B operand of the forward, lane (class l31, k half lh): read from a block-wide LDS copy of the codes at every k-step (row pitch 528
  // bytes: the 16-byte reads of 32 consecutive rows fall on different banks).  Held in registers, its 64 VGPRs on top of the 128
  // accumulators and the 64 of raw x pushed the kernel to 484 registers and ~700 AGPR copies per row group.
  for (int i = tid; i < 1024; i += 256)
    *reinterpret_cast<u32x4*>(wl + (i >> 5) * CG_W_PITCH + (i & 31) * 16) = *reinterpret_cast<const u32x4*>(w + (i >> 5) * 256 + (i & 31) * 8);
  __syncthreads();  // the only barrier: in front of every divergent path
  const float bs = bias[l31];
  const bool cls_on = l31 < nb;  // a padding column: zero code row, no loss, no gradient
  const int my_cls = n0 + l31;

  // transposed reads: lane 4 q + p of a 16-lane group addresses row r0 + q, channels c0 + 4 p .. + 3 of its block; the group's
  // block is rows 16 s + 8 jj + 4 lh .. + 3, channels 32 ct + 16 (group & 1) .. + 15
  const int tq = (lane >> 2) & 3, tp = lane & 3, tg = (lane >> 4) & 1;
  unsigned char* const img = xt[wave];

  const int n_groups = n_tiles * 4;
  const int n_units = (n_groups + CLS_GRAD_UNIT_GROUPS - 1) / CLS_GRAD_UNIT_GROUPS;
  for (int unit = blockIdx.x * 4 + wave; unit < n_units; unit += gridDim.x * 4) {
    f32x16 acc[8];  // dW^T: register r of tile ct = channel 32 ct + (r & 3) + 8 (r >> 2) + 4 lh of class l31
#pragma unroll
    for (int ct = 0; ct < 8; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
    float db = 0.f, loss = 0.f;
    int cur_seg = -1;
    const int g_end = min(n_groups, (unit + 1) * CLS_GRAD_UNIT_GROUPS);
    for (int g = unit * CLS_GRAD_UNIT_GROUPS; g < g_end; ++g) {
      const RowGroup rg = row_group(segs, tiles, g);
      if (rg.empty()) continue;  // wave-uniform
      if (rg.seg != cur_seg) {
        cur_seg = rg.seg;
        gn_load_coef(cf[wave], coef, rg.seg, lane);
      }
      const size_t grow = rg.grow(l31);
      const int lab = rg.valid(l31) ? labels[grow] : -2;  // -2: a row past the map -- computed, contributes nothing
      const bf16_t* xp = x + grow * ld + lh * 8;
      u32x4 xv[16];
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) xv[ks] = *reinterpret_cast<const u32x4*>(xp + ks * 16);
      f32x16 z;
#pragma unroll
      for (int r = 0; r < 16; ++r) z[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) {
        const u32x4 yv = gn_relu_x8(xv[ks], cf[wave], ks, lh);
        *reinterpret_cast<u32x4*>(img + xt_off(l31, 2 * ks + lh)) = yv;
        const bf16x8 wf = *reinterpret_cast<const bf16x8*>(wl + l31 * CG_W_PITCH + ks * 32 + lh * 16);
        z = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, yv), wf, z, 0, 0, 0);
      }
      // loss and g on the lane's 16 positions of its class
      s16x8 ghi[2], glo[2];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int p = (r & 3) + 8 * (r >> 2) + 4 * lh;
        const int lp = __shfl(lab, p);
        float l1, g1;
        focal_one(z[r] + bs, lp == my_cls, alpha, gamma, l1, g1);
        const bool on = cls_on && lp != -2;
        l1 = on ? l1 : 0.f;
        g1 = on ? g1 : 0.f;
        loss += l1;
        db += g1;
        const bf16_t h = (bf16_t)g1;
        const bf16_t l = (bf16_t)(g1 - (float)h);
        ghi[r >> 3][r & 7] = __builtin_bit_cast(short, h);
        glo[r >> 3][r & 7] = __builtin_bit_cast(short, l);
      }
      // dW^T += xn^T g
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int ct = 0; ct < 8; ++ct) {
          s16x4 a[2];
#pragma unroll
          for (int jj = 0; jj < 2; ++jj) {
            const int row = 16 * s + 8 * jj + 4 * lh + tq;
            a[jj] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(img + xt_off(row, 4 * ct + 2 * tg + (tp >> 1)) + 8 * (tp & 1)));
          }
          const s16x8 av = {a[0][0], a[0][1], a[0][2], a[0][3], a[1][0], a[1][1], a[1][2], a[1][3]};
          acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, ghi[s]), acc[ct], 0, 0, 0);
          acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, glo[s]), acc[ct], 0, 0, 0);
        }
    }
    // the unit's partial
    float* pp = part + (size_t)unit * CLS_GRAD_PARTIAL;
#pragma unroll
    for (int ct = 0; ct < 8; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) pp[(32 * ct + (r & 3) + 8 * (r >> 2) + 4 * lh) * 32 + l31] = acc[ct][r];
    db += __shfl_xor(db, 32);
    for (int o = 32; o > 0; o >>= 1) loss += __shfl_xor(loss, o);
    if (lh == 0) pp[8192 + l31] = db;
    if (lane == 0) pp[8224] = loss;
  }
}

// the sink of the tree's final kernel: element i of the summed partial -> grad_w[nb][256], grad_b[nb] (nullptr: none), loss (accumulate:
// added to what the earlier class blocks of the call left there)
struct ClsGradSink {
  int nb;
  float *grad_w, *grad_b, *loss;
  int accumulate;
  __device__ void operator()(int i, float s) const {
    if (i < 8192) {
      const int c = i >> 5, n = i & 31;
      if (n < nb) grad_w[n * 256 + c] = s;
    } else if (i < 8224) {
      if (grad_b && i - 8192 < nb) grad_b[i - 8192] = s;
    } else {
      *loss = accumulate ? *loss + s : s;
    }
  }
};

int cls_grad_units(int n_tiles) { return (n_tiles * 4 + CLS_GRAD_UNIT_GROUPS - 1) / CLS_GRAD_UNIT_GROUPS; }

// floats of workspace for one class block: the units' partials and every level of their sums
size_t cls_grad_ws_floats(int n_tiles) { return partial_tree(cls_grad_units(n_tiles), CLS_GRAD_FANIN).planes * CLS_GRAD_PARTIAL; }

// w: [32][256] bf16 (rows >= nb zero), bias: [32] fp32; ws: cls_grad_ws_floats(n_tiles) floats; grad_w: [nb][256], grad_b: [nb] or nullptr
int launch_cls_grad(const void* x, int ld, const float2* coef, const void* w, const float* bias, int nb, int n0, const int* labels, float alpha,
                    float gamma, float* ws, float* loss, int accumulate, float* grad_w, float* grad_b, const SegDesc* segs, const int2* tiles,
                    int n_tiles, hipStream_t s) {
  if (nb < 1 || nb > 32 || n_tiles <= 0 || !bias || !ws) return -1;
  const int n = cls_grad_units(n_tiles), blocks = (n + 3) / 4;
  // SYLPH_CLS_GRAD_BLOCKS: another block cap (tests: a wave then takes several units; the results must keep their bits)
  const int cap = block_cap("SYLPH_CLS_GRAD_BLOCKS", CLS_GRAD_MAX_BLOCKS);
  hipLaunchKernelGGL(cls_grad_kernel, dim3(blocks < cap ? blocks : cap), dim3(256), 0, s, (const bf16_t*)x, ld, coef,
                     (const bf16_t*)w, bias, nb, n0, labels, alpha, gamma, ws, segs, tiles, n_tiles);
  partial_final(partial_sum_passes(ws, n, CLS_GRAD_PARTIAL, CLS_GRAD_FANIN, s), CLS_GRAD_PARTIAL, 8225,
                ClsGradSink{nb, grad_w, grad_b, loss, accumulate}, s);
  return (int)hipGetLastError();
}

}  // namespace sylph
