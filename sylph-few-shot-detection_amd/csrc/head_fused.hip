// GroupNorm + ReLU of the cls tower's last layer fused into the class-conditional 1x1 conv (N <= 32 classes), bf16.
//
//   logits[row][n] = sum_c bf16(relu(a[seg][c] * x[row][c] + b[seg][c])) * W[n][c] + bias[n]
//
// Reference ops: the last `GroupNorm(32, 256)` + `ReLU` of `MetaFCOSHead.cls_tower` followed by `CondConvBasic`
// (sylph/modeling/meta_fcos/fcos.py:582-667, head_utils.py:60-81).  Unfused, the normalised tensor is written by
// gn_apply_partials_kernel and read back by the 128x32 conv_igemm launch (2 x 734 MB at B = 64); nobody else reads it.  Here
// every wave streams 32-row groups straight from HBM into MFMA A-fragment registers (lane = (row, k half): 16 bytes per
// k-step, a row's 512 bytes over 16 k-steps), applies the same fused multiply-add + ReLU + bf16 rounding as the apply kernel
// (bit-identical operand values), and multiplies by the 32 x 256 code matrix held in registers.  No LDS for data, no barriers:
// the pass is HBM-bound (one read of the tower output, one write of the fp32 logits).  The row-group walk, the coefficient table and the
// normalisation are gn_stream.h's, shared with every kernel below that says its operand values are this kernel's, and with
// logits_scan_kernel (detect.hip).
//
// EPISODES (sylph_fcos_head_episodes; the loop the batch stands for: meta_learn_evaluation.py:421-426): the images of the batch belong
// to different episodes.  w / bias hold every episode's block of 32 rows (zero rows and zero biases above its N), seg_row0[segment] is
// the first row of the block of the segment's image: tile -> segment -> image -> episode -> code rows.  A wave reloads its B fragments
// and biases only when the block of its next tile differs from the one it holds; everything else -- operand values, K order, rounding
// points -- is the uniform kernel's, so an image's logits do not depend on which episodes its neighbours belong to.
#include "gn_stream.h"
#include "kernels.h"

namespace sylph {

template <bool EPISODES>
__global__ __launch_bounds__(256) void gn_logits_kernel(const bf16_t* __restrict__ x, int ld, const float2* __restrict__ coef,
                                                        const bf16_t* __restrict__ w, const float* __restrict__ bias, int N,
                                                        const int* __restrict__ seg_row0, float* __restrict__ out, int out_ld,
                                                        const SegDesc* __restrict__ segs, const int2* __restrict__ tiles, int n_tiles) {
  __shared__ __attribute__((aligned(16))) float cf[4][512];  // per wave: (a0, a1, b0, b1) per channel pair of its current segment
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;

  bf16x8 Wf[16];  // B operand: lane (n = l31, k half lh)
  float bs[16];   // D^T: register 4q + e of a lane is class 8q + 4lh + e of row l31
  auto load_codes = [&](int row0) {  // the 32 x 256 block that starts at packed row row0
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) Wf[ks] = *reinterpret_cast<const bf16x8*>(w + (size_t)(row0 + l31) * 256 + ks * 16 + lh * 8);
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int n = 8 * q + 4 * lh + e;
        bs[4 * q + e] = (bias && n < N) ? bias[row0 + n] : 0.f;
      }
  };
  int cur_row0 = EPISODES ? -1 : 0;
  if constexpr (!EPISODES) load_codes(0);

  int cur_seg = -1;
  // uniform: a block takes every gridDim.x-th tile.  EPISODES: a block takes a contiguous run of tiles -- its waves then stay inside one
  // image (a few hundred tiles) for nearly all of it, and a code block is loaded once or twice per wave instead of once per tile
  const int chunk = EPISODES ? (n_tiles + (int)gridDim.x - 1) / (int)gridDim.x : 1;
  const int n_groups = EPISODES ? min(n_tiles, ((int)blockIdx.x + 1) * chunk) * 4 : n_tiles * 4;
  const int stride = EPISODES ? 4 : gridDim.x * 4;
  for (int g = blockIdx.x * chunk * 4 + wave; g < n_groups; g += stride) {
    const RowGroup rg = row_group(segs, tiles, g);
    if (rg.empty()) continue;
    if (rg.seg != cur_seg) {          // wave-private coefficient table
      cur_seg = rg.seg;
      if constexpr (EPISODES) {
        const int row0 = seg_row0[rg.seg];  // wave-uniform
        if (row0 != cur_row0) { cur_row0 = row0; load_codes(row0); }
      }
      gn_load_coef(cf[wave], coef, rg.seg, lane);
    }
    const bool valid = rg.valid(l31);
    const size_t grow = rg.grow(l31);
    const bf16_t* xp = x + grow * ld + lh * 8;
    u32x4 xv[16];
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) xv[ks] = *reinterpret_cast<const u32x4*>(xp + ks * 16);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 16; ++ks)
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Wf[ks], __builtin_bit_cast(bf16x8, gn_relu_x8(xv[ks], cf[wave], ks, lh)), acc, 0, 0, 0);
    if (valid) {
      float* op = out + grow * out_ld + 4 * lh;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (8 * q + 4 * lh < out_ld)  // out_ld: any multiple of 4 >= N (8 for <= 8 classes)
          *reinterpret_cast<float4*>(op + 8 * q) =
              make_float4(acc[4 * q] + bs[4 * q], acc[4 * q + 1] + bs[4 * q + 1], acc[4 * q + 2] + bs[4 * q + 2], acc[4 * q + 3] + bs[4 * q + 3]);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The same pass for SEVERAL code sets over the same images (sylph_fcos_head_codesets; the loop it stands for: one query pass per
// support seed, meta_fcos_runner.py:451-672, or one per tenant of a served frame).  Everything in front of the class-conditional conv is
// class-agnostic (fcos.py:582-667, head_utils.py:60-81), so a 32-row group of the tower output is read from HBM and normalised ONCE
// and multiplied by NB blocks of 32 code rows held in registers: NB MFMAs per k-step into NB accumulators.  Operand load,
// fma -> bf16 -> ReLU rounding point, K order and mfma_f32_32x32x16_bf16 are gn_logits_kernel's, and an MFMA output element depends on
// its own code row and activation row only -- not on the column it sits in -- so a class's logits are bit for bit those of the
// one-set kernel wherever its row lies in the packed table; a set may straddle two blocks.
// w: [32 NB][256] bf16 (zero rows where no class sits), bias: as many fp32 (zeros without a bias); column n of the launch is packed
// row n, written at out[row][n] for n < width (a multiple of 4).  The NB x 64 registers of code fragments, 64 of raw x and NB x 16
// accumulators fit the 512-register file of one wave per SIMD (NB = 4: no scratch in the compiler's resource report).
template <int NB>
__global__ __launch_bounds__(256) void gn_logits_sets_kernel(const bf16_t* __restrict__ x, int ld, const float2* __restrict__ coef,
                                                             const bf16_t* __restrict__ w, const float* __restrict__ bias,
                                                             float* __restrict__ out, int out_ld, int width,
                                                             const SegDesc* __restrict__ segs, const int2* __restrict__ tiles, int n_tiles) {
  __shared__ __attribute__((aligned(16))) float cf[4][512];  // per wave: (a0, a1, b0, b1) per channel pair of its current segment
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;

  bf16x8 Wf[NB][16];  // lane (n = 32 b + l31, k half lh): loaded once, the code blocks never change within a launch
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) Wf[b][ks] = *reinterpret_cast<const bf16x8*>(w + (size_t)(32 * b + l31) * 256 + ks * 16 + lh * 8);

  int cur_seg = -1;
  const int n_groups = n_tiles * 4, stride = gridDim.x * 4;
  for (int g = blockIdx.x * 4 + wave; g < n_groups; g += stride) {
    const RowGroup rg = row_group(segs, tiles, g);
    if (rg.empty()) continue;
    if (rg.seg != cur_seg) {          // wave-private coefficient table, carried from one row group to the next
      cur_seg = rg.seg;
      gn_load_coef(cf[wave], coef, rg.seg, lane);
    }
    const bool valid = rg.valid(l31);
    const size_t grow = rg.grow(l31);
    const bf16_t* xp = x + grow * ld + lh * 8;
    u32x4 xv[16];
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) xv[ks] = *reinterpret_cast<const u32x4*>(xp + ks * 16);
    f32x16 acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
      const bf16x8 yv = __builtin_bit_cast(bf16x8, gn_relu_x8(xv[ks], cf[wave], ks, lh));
#pragma unroll
      for (int b = 0; b < NB; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Wf[b][ks], yv, acc[b], 0, 0, 0);
    }
    if (valid) {
      float* op = out + grow * out_ld + 4 * lh;
      const float* bp = bias + 4 * lh;
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int n = 32 * b + 8 * q;  // D^T: register 4q + e of a lane is column 32 b + 8 q + 4 lh + e of row l31
          if (n + 4 * lh < width) {
            const float4 b4 = *reinterpret_cast<const float4*>(bp + n);  // (L2 hits: the biases are not worth 16 NB registers)
            *reinterpret_cast<float4*>(op + n) =
                make_float4(acc[b][4 * q] + b4.x, acc[b][4 * q + 1] + b4.y, acc[b][4 * q + 2] + b4.z, acc[b][4 * q + 3] + b4.w);
          }
        }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Last GroupNorm + ReLU of the bbox tower fused into the 3x3 prediction convs (bbox_pred 4 + ctrness 1 [+ iou 1] channels).
// A 3x3 conv with a handful of output channels is linear in its taps:
//     pred[r][n] = sum_tap ( xn[r + shift(tap)] . W[tap][n] ),     xn = relu(GN(x)),  zero outside the map,
// so pass 1 streams xn ONCE (same HBM -> register scheme as gn_logits_kernel) against the 9 * Cp <= 64 stacked tap rows and
// writes the per-position tap responses (fp32, <= 64 per position); pass 2 adds the nine shifted responses, bias, per-level
// Scale and ReLU (`F.relu(scale_l(bbox_pred(t)))`, fcos.py:640-660).  Unfused: apply (0.73 GB read + 0.73 GB write) + a halo-mode
// 128x32 conv (0.73 GB read); fused: 0.73 GB read + 0.28 GB write + 0.28 GB read.
template <int NT>
__global__ __launch_bounds__(256) void gn_taps_kernel(const bf16_t* __restrict__ x, int ld, const float2* __restrict__ coef,
                                                      const bf16_t* __restrict__ w, float* __restrict__ out, int sw, size_t plane_rows,
                                                      const SegDesc* __restrict__ segs, const int2* __restrict__ tiles, int n_tiles) {
  __shared__ __attribute__((aligned(16))) float cf[4][512];
  constexpr int TR_PITCH = NT * 32 + 4;  // floats per row of the transpose tile (+4: the 16-byte row pieces of 8 lanes fall on different banks)
  __shared__ __attribute__((aligned(16))) float tr[4][32 * TR_PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
  bf16x8 Wf[NT][16];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) Wf[t][ks] = *reinterpret_cast<const bf16x8*>(w + (t * 32 + l31) * 256 + ks * 16 + lh * 8);
  int cur_seg = -1;
  const int n_groups = n_tiles * 4, stride = gridDim.x * 4;
  for (int g = blockIdx.x * 4 + wave; g < n_groups; g += stride) {
    const RowGroup rg = row_group(segs, tiles, g);
    if (rg.empty()) continue;
    if (rg.seg != cur_seg) {
      cur_seg = rg.seg;
      gn_load_coef(cf[wave], coef, rg.seg, lane);
    }
    const bf16_t* xp = x + rg.grow(l31) * ld + lh * 8;
    u32x4 xv[16];
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) xv[ks] = *reinterpret_cast<const u32x4*>(xp + ks * 16);
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
      const bf16x8 yv = __builtin_bit_cast(bf16x8, gn_relu_x8(xv[ks], cf[wave], ks, lh));
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Wf[t][ks], yv, acc[t], 0, 0, 0);
    }
    // column j = kh * sw + kw * cp + n (sw = slice width, a multiple of 4): columns [kh sw, (kh + 1) sw) of a row are its record in
    // plane kh, so that pass 2 reads near-contiguous sw-float records per kernel row.  The 32 rows of the group are contiguous in
    // every plane (32 * sw floats): the accumulator tile is transposed through wave-private LDS and written as whole 16-byte
    // pieces of that run, 1 KiB per store instruction (direct from the accumulator layout a store touched 32 records for 32 bytes each).
    float* st = &tr[wave][0];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        *reinterpret_cast<float4*>(st + l31 * TR_PITCH + t * 32 + 8 * q + 4 * lh) =
            make_float4(acc[t][4 * q], acc[t][4 * q + 1], acc[t][4 * q + 2], acc[t][4 * q + 3]);
    const int vrows = min(32, rg.nrows - rg.r0), q4 = sw >> 2;
    const size_t grow0 = (size_t)rg.sd->out_row0 + rg.r0;
    for (int kh = 0; kh < 3; ++kh) {
      float* dst = out + ((size_t)kh * plane_rows + grow0) * sw;
      for (int i = lane; i < vrows * q4; i += 64) {
        const int row = i / q4, c4 = i - row * q4;
        *reinterpret_cast<float4*>(dst + (size_t)i * 4) = *reinterpret_cast<const float4*>(st + row * TR_PITCH + kh * sw + c4 * 4);
      }
    }
  }
}

// pass 2: block = one 128-row tile, one thread per output position.  For kernel row kh the tile needs the 130 CONTIGUOUS records
// [r0 + (kh - 1) W - 1, r0 + (kh - 1) W + 128] of plane kh: staged through LDS with coalesced float4 loads (pitch sw + 1 floats:
// conflict-free column reads); positions outside the map are masked at use (their records belong to other rows / segments).
__global__ __launch_bounds__(128) void tap_gather_kernel(const float* __restrict__ planes, int sw, size_t plane_rows, int cp,
                                                         const float* __restrict__ bias, int relu_nch, int mul_nch, float* __restrict__ out,
                                                         int out_ld, const SegDesc* __restrict__ segs, const int2* __restrict__ tiles) {
  __shared__ float sm[3][130 * 25];  // sw <= 24
  const int2 tl = tiles[blockIdx.x];
  const SegDesc& sd = segs[tl.x];
  const int H = sd.out_H, W = sd.out_W, HWn = H * W, r0 = tl.y, tid = threadIdx.x, pitch = sw + 1;
  const int q4 = sw >> 2;  // float4s per record
  // all of a thread's loads (<= 3 x 7 float4: sw <= 24 -> q4 <= 6, ceil(130 * 6 / 128) = 7) are issued before the first LDS store:
  // the staging is a pure HBM stream, and one load per loop trip was latency-bound (2.1 TB/s)
  constexpr int MAXIT = 7;
  float4 v[3][MAXIT];
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int first = r0 + (kh - 1) * W - 1;  // map-relative row of LDS record 0
    const float* pl = planes + ((size_t)kh * plane_rows + sd.out_row0) * sw;
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int i = tid + it * 128;
      const int rec = i / q4, c4 = i - rec * q4;
      const int rr = first + rec;
      v[kh][it] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (i < 130 * q4 && (unsigned)rr < (unsigned)HWn) v[kh][it] = *reinterpret_cast<const float4*>(pl + (size_t)rr * sw + c4 * 4);
    }
  }
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int i = tid + it * 128;
      if (i < 130 * q4) {
        const int rec = i / q4, c4 = i - rec * q4;
        float* d = &sm[kh][rec * pitch + c4 * 4];
        d[0] = v[kh][it].x; d[1] = v[kh][it].y; d[2] = v[kh][it].z; d[3] = v[kh][it].w;
      }
    }
  }
  __syncthreads();
  const int r = r0 + tid;
  if (r >= HWn) return;
  const int y = r / W, xx = r - y * W;
  float acc[8];
#pragma unroll
  for (int n = 0; n < 8; ++n) acc[n] = 0.f;
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {  // fixed order: kh outer, kw inner
    if ((unsigned)(y + kh - 1) >= (unsigned)H) continue;
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      if ((unsigned)(xx + kw - 1) >= (unsigned)W) continue;
      const float* tp = &sm[kh][(tid + kw) * pitch + kw * cp];  // record of row r + (kh - 1) W + (kw - 1)
#pragma unroll
      for (int n = 0; n < 8; ++n)
        if (n < cp) acc[n] += tp[n];
    }
  }
  float* op = out + (size_t)(sd.out_row0 + r) * out_ld;
#pragma unroll
  for (int n = 0; n < 8; ++n) {
    if (n >= cp) break;
    float t = acc[n] + bias[n];
    if (n < mul_nch) t *= sd.mul;
    if (n < relu_nch) t = t > 0.f ? t : 0.f;
    op[n] = t;
  }
}

// w_taps: [64][256] bf16, row kh * sw + kw * cp + n = W[n][kh][kw][:] with sw = roundup4(3 * cp) (other rows zero);
// planes_ws: fp32 [3][plane_rows][sw]
int launch_gn_pred_taps(const void* x, int ld, const float2* coef, const void* w_taps, int cp, const float* bias, int relu_nch, int mul_nch,
                        float* planes_ws, size_t plane_rows, float* out, int out_ld, const SegDesc* segs, const int2* tiles, int n_tiles,
                        hipStream_t s) {
  const int sw = (3 * cp + 3) & ~3;
  if (cp < 1 || 3 * sw > 64 || n_tiles <= 0) return -1;
  hipLaunchKernelGGL(gn_taps_kernel<2>, dim3(head_stream_grid(n_tiles)), dim3(256), 0, s, (const bf16_t*)x, ld, coef, (const bf16_t*)w_taps, planes_ws, sw, plane_rows,
                     segs, tiles, n_tiles);
  hipLaunchKernelGGL(tap_gather_kernel, dim3(n_tiles), dim3(128), 0, s, planes_ws, sw, plane_rows, cp, bias, relu_nch, mul_nch, out, out_ld, segs,
                     tiles);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// Last GroupNorm + ReLU of the cls tower fused into a 3x3 class-conditional conv (CODE_GENERATOR.CLS_LAYER kernel size 3, N <= 32), bf16:
//
//   logits[p][n] = sum_(ky, kx) sum_c xn[p + (ky - 1) W + (kx - 1)][c] * W[n][ky][kx][c] + bias[n],   xn = bf16(relu(a x + b))
//
// `F.conv2d(cls_tower, W, bias, padding = 1)` of CondConvBasic (head_utils.py:60-81, fcos.py:499-510): a cross-correlation whose zero
// padding applies to the NORMALISED tensor -- a tap whose source lies outside the (image, level) map contributes zero, not relu(b).
// The operand values are gn_logits_kernel's (same fma, same rounding point); xn is never written to HBM.  The nine taps' B fragments are
// 9 x 64 VGPRs, more than one wave has: a block is THREE waves, wave ky holds the three taps of kernel row ky (192 VGPRs) and walks the
// same 32-position groups as its siblings.  For a group at map-relative rows [r0, r0 + 32) the taps of kernel row ky read the 34
// CONTIGUOUS rows [r0 + (ky - 1) W - 1, r0 + (ky - 1) W + 33): the wave loads that strip once (coalesced 16-byte pieces: a lane keeps one
// 8-channel column of the strip, so its 16 GroupNorm coefficients live in registers), normalises it once and leaves it in wave-private
// LDS; tap kx of output row j is strip row j + kx (row pitch 528 bytes: the 16-byte operand reads of 32 consecutive rows fall on
// different banks).  A strip row outside the map is clamped to a valid row: every output that would read it is masked.  Each tap has
// its own accumulator; in the D^T layout a lane holds ONE position's 16 classes, so the zero padding is a per-lane select of whole
// accumulators (tap row outside the map: all three; column -1 / W: the kx = 0 / 2 one).  The next group's strip is loaded while the
// MFMAs of the current one run.  The three kernel rows' 32 x 32 partials are summed in the fixed order ky = 0, 1, 2 through LDS (two
// buffers, one barrier per group) and wave 0 writes the logits once.
constexpr int C3_PITCH = 528;  // bytes per strip row in LDS
__global__ __launch_bounds__(192) void gn_cond3x3_kernel(const bf16_t* __restrict__ x, int ld, const float2* __restrict__ coef,
                                                         const bf16_t* __restrict__ w, const float* __restrict__ bias, int N,
                                                         float* __restrict__ out, int out_ld, const SegDesc* __restrict__ segs,
                                                         const int2* __restrict__ tiles, int n_tiles) {
  __shared__ __attribute__((aligned(16))) unsigned char strip[3][34 * C3_PITCH];  // per wave: the normalised strip of its current group
  __shared__ __attribute__((aligned(16))) float red[2][2][1024];                   // [group parity][wave 1 | 2]: register r of lane l at r * 64 + l
  const int tid = threadIdx.x, lane = tid & 63, ky = tid >> 6, l31 = lane & 31, lh = lane >> 5;
  bf16x8 Wf[3][16];  // B operands of taps (ky, 0..2): lane (n = l31, k half lh)
#pragma unroll
  for (int kx = 0; kx < 3; ++kx)
#pragma unroll
    for (int ks = 0; ks < 16; ++ks)
      Wf[kx][ks] = *reinterpret_cast<const bf16x8*>(w + ((size_t)l31 * 9 + ky * 3 + kx) * 256 + ks * 16 + lh * 8);
  float bs[16];  // D^T: register 4q + e of a lane is class 8q + 4lh + e of row l31
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int n = 8 * q + 4 * lh + e;
      bs[4 * q + e] = (bias && n < N) ? bias[n] : 0.f;
    }
  const int end = n_tiles * 4;
  // the groups of a block: the four of a tile, then the tile one grid stride on; groups past the end of a short level are skipped
  // (block-uniform: the three waves walk the same groups)
  auto group_r0 = [&](int g) { return tiles[g >> 2].y + (g & 3) * 32; };
  auto group_rows = [&](int g) { const SegDesc& sd = segs[tiles[g >> 2].x]; return sd.out_H * sd.out_W; };
  auto next_group = [&](int g) {
    do g = (g & 3) == 3 ? g - 3 + (int)gridDim.x * 4 : g + 1;
    while (g < end && group_r0(g) >= group_rows(g));
    return g;
  };
  // a lane's pieces of a strip: piece it * 64 + lane = (strip row 2 it + lh, 8-channel column l31), 17 pieces = 34 rows
  u32x4 xv[17];
  auto load_strip = [&](int g) {
    const SegDesc& sd = segs[tiles[g >> 2].x];
    const int nrows = sd.out_H * sd.out_W, first = group_r0(g) + (ky - 1) * sd.out_W - 1;
    const bf16_t* base = x + (size_t)sd.out_row0 * ld + l31 * 8;
#pragma unroll
    for (int it = 0; it < 17; ++it) {
      const int r = min(max(first + 2 * it + lh, 0), nrows - 1);
      xv[it] = *reinterpret_cast<const u32x4*>(base + (size_t)r * ld);
    }
  };
  f32x2 ca[4], cb[4];  // (a, b) of the lane's 8 channels, as pairs
  int cur_seg = -1, par = 0;
  int g = blockIdx.x * 4;  // (the first group of a tile is never empty)
  if (g < end) load_strip(g);
  while (g < end) {
    const int seg = tiles[g >> 2].x, r0 = group_r0(g);
    const SegDesc& sd = segs[seg];
    const int Hm = sd.out_H, Wm = sd.out_W, nrows = Hm * Wm;
    if (seg != cur_seg) {
      cur_seg = seg;
      const float2* cp = coef + (size_t)seg * 256 + l31 * 8;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float2 c0 = cp[2 * e], c1 = cp[2 * e + 1];
        ca[e] = f32x2{c0.x, c1.x};
        cb[e] = f32x2{c0.y, c1.y};
      }
    }
    // normalise the strip once: bf16(relu(fma(a, x, b))) -> LDS
#pragma unroll
    for (int it = 0; it < 17; ++it) {
      u32x4 yv;
#pragma unroll
      for (int e = 0; e < 4; ++e) yv[e] = gn_relu_pair(xv[it][e], ca[e], cb[e]);
      *reinterpret_cast<u32x4*>(&strip[ky][(2 * it + lh) * C3_PITCH + l31 * 16]) = yv;
    }
    const int gn = next_group(g);
    if (gn < end) load_strip(gn);  // in flight under the MFMAs below
    f32x16 acc[3];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[kx][r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 16; ++ks)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const bf16x8 yv = *reinterpret_cast<const bf16x8*>(&strip[ky][(l31 + kx) * C3_PITCH + ks * 32 + lh * 16]);
        acc[kx] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Wf[kx][ks], yv, acc[kx], 0, 0, 0);
      }
    // zero padding of the normalised tensor, per position = per lane
    const int row = r0 + l31;
    const bool valid = row < nrows;
    const int own = valid ? row : nrows - 1;
    const int py = own / Wm, px = own - py * Wm;
    const bool mrow = valid && (unsigned)(py + ky - 1) < (unsigned)Hm;
    const bool m0 = mrow && px > 0, m2 = mrow && px < Wm - 1;
    f32x16 sum;
#pragma unroll
    for (int r = 0; r < 16; ++r) sum[r] = ((m0 ? acc[0][r] : 0.f) + (mrow ? acc[1][r] : 0.f)) + (m2 ? acc[2][r] : 0.f);
    if (ky != 0) {
      float* rp = &red[par][ky - 1][lane];
#pragma unroll
      for (int r = 0; r < 16; ++r) rp[r * 64] = sum[r];
    }
    __syncthreads();
    if (ky == 0 && valid) {
      const float *r1 = &red[par][0][lane], *r2 = &red[par][1][lane];
      float* op = out + (size_t)(sd.out_row0 + row) * out_ld + 4 * lh;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (8 * q + 4 * lh < out_ld) {  // out_ld: any multiple of 4 >= N (8 for <= 8 classes)
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = (sum[4 * q + e] + r1[(4 * q + e) * 64]) + r2[(4 * q + e) * 64] + bs[4 * q + e];
          *reinterpret_cast<float4*>(op + 8 * q) = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
    par ^= 1;  // the next group's partials go to the other buffer: wave 0 may still be reading this one
    g = gn;
  }
}

// x: raw (un-normalised) tower output [rows][ld] bf16; coef: [segments][256] (a, b); w: [32][3][3][256] bf16 (rows >= N zero);
// out: fp32 [rows][out_ld], out_ld a multiple of 4 >= N; segs / tiles: the 128-row pointwise tile table of the head
int launch_gn_cond3x3(const void* x, int ld, const float2* coef, const void* w, const float* bias, int N, float* out, int out_ld,
                      const SegDesc* segs, const int2* tiles, int n_tiles, hipStream_t s) {
  if (N > 32 || out_ld < N || (out_ld & 3) != 0 || n_tiles <= 0) return -1;
  hipLaunchKernelGGL(gn_cond3x3_kernel, dim3(head_stream_grid(n_tiles)), dim3(192), 0, s, (const bf16_t*)x, ld, coef, (const bf16_t*)w, bias, N, out, out_ld, segs,
                     tiles, n_tiles);
  return (int)hipGetLastError();
}

// x: raw (un-normalised) tower output [rows][ld] bf16; coef: [segments][256] (a, b); w: [32][256] bf16 (rows >= N zero);
// out: fp32 [rows][out_ld], out_ld a multiple of 4 >= N; segs / tiles: the 128-row pointwise tile table of the head
int launch_gn_logits(const void* x, int ld, const float2* coef, const void* w, const float* bias, int N, float* out, int out_ld,
                     const SegDesc* segs, const int2* tiles, int n_tiles, hipStream_t s) {
  if (N > 32 || out_ld < N || (out_ld & 3) != 0 || n_tiles <= 0) return -1;
  hipLaunchKernelGGL(gn_logits_kernel<false>, dim3(head_stream_grid(n_tiles)), dim3(256), 0, s, (const bf16_t*)x, ld, coef, (const bf16_t*)w, bias, N, nullptr, out,
                     out_ld, segs, tiles, n_tiles);
  return (int)hipGetLastError();
}

// w: [32 * nblocks][256] bf16, bias: as many fp32 (never null: zeros without a bias), nblocks in 1 .. 4; out: fp32 [rows][out_ld], columns
// [0, width) written, width a multiple of 4 in (32 (nblocks - 1), 32 nblocks], out_ld a multiple of 4 >= width
int launch_gn_logits_sets(const void* x, int ld, const float2* coef, const void* w, const float* bias, int nblocks, float* out, int out_ld,
                          int width, const SegDesc* segs, const int2* tiles, int n_tiles, hipStream_t s) {
  if (nblocks < 1 || nblocks > GN_SETS_MAX_BLOCKS || !bias || width <= 32 * (nblocks - 1) || width > 32 * nblocks || (width & 3) != 0 ||
      out_ld < width || (out_ld & 3) != 0 || n_tiles <= 0)
    return -1;
  const int grid = head_stream_grid(n_tiles);
#define SYLPH_SETS_LAUNCH(NB)                                                                                                            \
  hipLaunchKernelGGL(gn_logits_sets_kernel<NB>, dim3(grid), dim3(256), 0, s, (const bf16_t*)x, ld, coef, (const bf16_t*)w, bias, out, \
                     out_ld, width, segs, tiles, n_tiles)
  switch (nblocks) {
    case 1: SYLPH_SETS_LAUNCH(1); break;
    case 2: SYLPH_SETS_LAUNCH(2); break;
    case 3: SYLPH_SETS_LAUNCH(3); break;
    default: SYLPH_SETS_LAUNCH(4); break;
  }
#undef SYLPH_SETS_LAUNCH
  return (int)hipGetLastError();
}

// w: [32 * episodes][256] bf16, bias: as many fp32 (nullptr: no bias), both zero above each episode's N; seg_row0: [segments]
int launch_gn_logits_episodes(const void* x, int ld, const float2* coef, const void* w, const float* bias, const int* seg_row0, float* out,
                              int out_ld, const SegDesc* segs, const int2* tiles, int n_tiles, hipStream_t s) {
  if (!seg_row0 || (out_ld & 3) != 0 || out_ld <= 0 || n_tiles <= 0) return -1;
  hipLaunchKernelGGL(gn_logits_kernel<true>, dim3(head_stream_grid(n_tiles)), dim3(256), 0, s, (const bf16_t*)x, ld, coef, (const bf16_t*)w, bias, 32, seg_row0, out,
                     out_ld, segs, tiles, n_tiles);
  return (int)hipGetLastError();
}

}  // namespace sylph
