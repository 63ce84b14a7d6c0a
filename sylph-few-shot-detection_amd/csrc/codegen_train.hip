// Meta-training of the Sylph hypernetwork (the CodeGenerator) on a frozen detector, bf16: the training-mode forward of
// CodeGeneratorHead.forward_roi_align (code_generator.py:924-1002 with :766-875) on a bank of constant ROI maps, and its backward from
// d loss / d (normalised code, processed bias) down to every generator parameter.  Parameters are the caller's fp32 master copies in one
// flat vector (cgt_param_layout); R = 49 M rows, row r = position r % 49 of shot r / 49, shot s reads bank row idx[s].
//
// forward   cgt_pack_kernel      fp32 (Cout, 256, 3, 3) -> bf16 [co][tap][ci] (the conv operand, rounded as pack_conv rounds it); for a tower
//                                layer also [ci][8 - tap][co], the operand of its data gradient; for the cls head also [tap ci][co]
//           cgt_conv_kernel      3x3 conv over the 7x7 maps as an implicit GEMM on 16x16x32 bf16 MFMAs: rows x 2304 x 256, zero padding
//                                inside each map, fp32 out.  y_i = conv(x_i, W_i) + b_i
//           cgt_gn_fwd_kernel    GroupNorm(32) statistics of the fp32 y_i per (shot, group) -- two passes, fixed order -- saved as
//                                (mean, rstd); x_{i+1} = bf16(relu((y - mean) rstd gamma + beta))
//           cgt_xsum_kernel      the pool commutes with the conv: Xsum[s][tap][ci] = the box sum of x_L[s] over the positions tap reaches (fp32)
//           cgt_head_fwd_kernel  c[s] = Xsum[s] . bf16(W_cls)^T / 49 + b_cls,  rb[s] = Xsum[s] . bf16(W_bias) / 49 + b_bias   (VALU, fp32)
//           cgt_tail_fwd_kernel  one block per class: shot mean, post GroupNorm, L2 normalisation, the two scales, the prior (fp32)
// backward  cgt_tail_bwd_kernel  one block per class: d code_raw, d bias_raw, d c[s], d rb[s] and the class's terms of d post_norm,
//                                d conv_scale, d bias_scale; cgt_colsum_kernel adds the classes in order
//           cgt_head_wgrad_kernel  d W[co][k] = sum_s d c[s][co] Xsum[s][k] / 49 in ascending s
//           cgt_dxsum_kernel / cgt_scatter_kernel   d Xsum = d c . bf16(W_cls) / 49 (+ the bias head), scattered back to d x_L
//           cgt_gn_bwd_kernel    ReLU mask from the saved x_{i+1}, GroupNorm backward from the saved y_i / (mean, rstd): d y_i (fp32) and the
//                                shot's terms of d gamma_i, d beta_i, d b_i; cgt_colsum_kernel adds the shots in order
//           cgt_conv_kernel      d x_i = conv(bf16(d y_i), flipped transposed weights), layers 1 and up
//           cgt_wgrad_kernel     d W_i[co][tap][ci] = sum_rows bf16(d y_i)[row][co] x_i[row + tap][ci] on the MFMAs: the rows are cut into UNITS
//                                of CGT_UNIT_SHOTS whole shots, a function of M alone; a block stages 32 rows of both operands transposed
//                                in LDS per K step and writes the unit's partial; the ordered tree of partial_sum.h (fan-in CGT_FANIN) adds
//                                the partials and its sink here, CgtWgradSink, writes torch's (co, ci, ky, kx) layout
// No atomics anywhere: the same inputs give the same bits on every call and on every grid (SYLPH_CODEGEN_TRAIN_BLOCKS caps the blocks).
// Rounding points: conv weights and d y_i to bf16 at the operand, x_{i+1} stored in bf16; everything else fp32.  The gradient treats
// every rounding as the identity.
#include <stdlib.h>

#include "gfx950.h"
#include "kernels.h"
#include "partial_sum.h"

namespace sylph {

namespace {

constexpr int C = 256, NPOS = 49, K9 = 2304;

typedef float f32x4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool tap_ok(int py, int px, int tap) {
  const int ky = tap / 3, kx = tap - 3 * ky;
  return (unsigned)(py + ky - 1) < 7u && (unsigned)(px + kx - 1) < 7u;
}
__device__ __forceinline__ int tap_off(int tap) { return (tap / 3 - 1) * 7 + (tap % 3 - 1); }

// w (cout, 256, 3, 3) fp32 -> wf [co][tap][ci]; wd [ci][8 - tap][co] (cout == 256) and wt [tap ci][co] where given
__global__ __launch_bounds__(256) void cgt_pack_kernel(const float* __restrict__ w, int cout, bf16_t* __restrict__ wf, bf16_t* __restrict__ wd,
                                                       bf16_t* __restrict__ wt) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= cout * K9) return;
  const int co = i / K9, k = i - co * K9, tap = k >> 8, ci = k & 255;
  const bf16_t v = (bf16_t)w[w3x3_torch(co, tap, ci)];
  wf[i] = v;
  if (wd) wd[(size_t)ci * K9 + (8 - tap) * C + co] = v;
  if (wt) wt[(size_t)k * cout + co] = v;
}

template <typename T> __device__ __forceinline__ bf16x8 load_frag(const T* p);
template <> __device__ __forceinline__ bf16x8 load_frag<bf16_t>(const bf16_t* p) { return *reinterpret_cast<const bf16x8*>(p); }
template <> __device__ __forceinline__ bf16x8 load_frag<float>(const float* p) {
  float v[8];
  load8<float>(p, v);
  bf16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (bf16_t)v[e];
  return o;
}

// out[r][n] = bias[n] + sum over (tap, ci) of in[shot_map(r / 49) * 49 + r % 49 + tap][ci] wp[n][tap][ci], zero outside the 7x7 map.  A block
// of four waves takes tiles of 32 rows x 256 columns, wave w the columns [64 w, 64 w + 64): two position fragments x four weight fragments
template <typename TIn>
__global__ __launch_bounds__(256) void cgt_conv_kernel(const TIn* __restrict__ in, const int* __restrict__ shot_map, const bf16_t* __restrict__ wp,
                                                       const float* __restrict__ bias, float* __restrict__ out, int rows) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, lq = lane >> 4;
  const int n0 = wave * 64, n_tiles = (rows + 31) / 32;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    long src[2];
    unsigned mask[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = tile * 32 + 16 * i + l15;
      src[i] = 0; mask[i] = 0;
      if (r < rows) {
        const int s = r / NPOS, p = r - s * NPOS, py = p / 7, px = p - 7 * py;
        src[i] = (long)(shot_map ? shot_map[s] : s) * NPOS + p;
        for (int tap = 0; tap < 9; ++tap) mask[i] |= tap_ok(py, px, tap) ? 1u << tap : 0u;
      }
    }
    f32x4v acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4v{0.f, 0.f, 0.f, 0.f};
    for (int tap = 0; tap < 9; ++tap) {
      const int off = tap_off(tap);
#pragma unroll 2
      for (int c0 = 0; c0 < C; c0 += 32) {
        bf16x8 fa[2], fb[4];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          bf16x8 z;
#pragma unroll
          for (int e = 0; e < 8; ++e) z[e] = (bf16_t)0.f;
          fa[i] = (mask[i] >> tap) & 1u ? load_frag<TIn>(in + (size_t)(src[i] + off) * C + c0 + lq * 8) : z;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) fb[j] = *reinterpret_cast<const bf16x8*>(wp + (size_t)(n0 + 16 * j + l15) * K9 + tap * C + c0 + lq * 8);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);  // D^T
      }
    }
    // accumulator layout: position 16 i + l15, channels n0 + 16 j + 4 lq .. + 3
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = tile * 32 + 16 * i + l15;
      if (r >= rows) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = n0 + 16 * j + 4 * lq;
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
        if (bias) b = *reinterpret_cast<const float4*>(bias + n);
        *reinterpret_cast<float4*>(out + (size_t)r * C + n) = make_float4(acc[i][j][0] + b.x, acc[i][j][1] + b.y, acc[i][j][2] + b.z, acc[i][j][3] + b.w);
      }
    }
  }
}

__device__ __forceinline__ float group8_sum(float v) {  // the 8 channels of a group are 8 consecutive lanes
  for (int o = 4; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// one block per shot, thread = channel
__global__ __launch_bounds__(256) void cgt_gn_fwd_kernel(const float* __restrict__ y, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         float2* __restrict__ stats, bf16_t* __restrict__ x) {
  const int s = blockIdx.x, c = threadIdx.x;
  const float* ys = y + (size_t)s * NPOS * C + c;
  float v[NPOS];
  float sum = 0.f;
#pragma unroll
  for (int p = 0; p < NPOS; ++p) { v[p] = ys[(size_t)p * C]; sum += v[p]; }
  const float mean = group8_sum(sum) / 392.f;
  float q = 0.f;
#pragma unroll
  for (int p = 0; p < NPOS; ++p) { const float d = v[p] - mean; q += d * d; }
  const float rstd = 1.0f / sqrtf(group8_sum(q) / 392.f + 1e-5f);
  if ((c & 7) == 0) stats[s * 32 + (c >> 3)] = make_float2(mean, rstd);
  const float ga = gamma[c], be = beta[c];
  bf16_t* xs = x + (size_t)s * NPOS * C + c;
#pragma unroll
  for (int p = 0; p < NPOS; ++p) xs[(size_t)p * C] = (bf16_t)fmaxf((v[p] - mean) * rstd * ga + be, 0.f);
}

// Xsum[s][tap][ci] = sum of x[s][q][ci] over the positions q = p + tap offset, p in the map, that lie in the map (ascending q)
__global__ __launch_bounds__(256) void cgt_xsum_kernel(const bf16_t* __restrict__ x, const int* __restrict__ shot_map, float* __restrict__ xsum) {
  const int s = blockIdx.x, c = threadIdx.x;
  const bf16_t* xs = x + (size_t)(shot_map ? shot_map[s] : s) * NPOS * C + c;
  float v[NPOS];
#pragma unroll
  for (int p = 0; p < NPOS; ++p) v[p] = (float)xs[(size_t)p * C];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int ky = tap / 3, kx = tap - 3 * ky;
    float a = 0.f;
#pragma unroll
    for (int qy = 0; qy < 7; ++qy)
#pragma unroll
      for (int qx = 0; qx < 7; ++qx)
        if ((unsigned)(qy - ky + 1) < 7u && (unsigned)(qx - kx + 1) < 7u) a += v[qy * 7 + qx];
    xsum[(size_t)s * K9 + tap * C + c] = a;
  }
}

// deterministic block sum of 256 values: wave butterflies, then the four wave sums in order
__device__ __forceinline__ float block_sum(float v, float* red4) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red4[0] + red4[1]) + red4[2]) + red4[3];
}

// one block per shot, thread = output channel
__global__ __launch_bounds__(256) void cgt_head_fwd_kernel(const float* __restrict__ xsum, const bf16_t* __restrict__ wht, const float* __restrict__ b,
                                                           const bf16_t* __restrict__ wb, const float* __restrict__ bb, float* __restrict__ cout,
                                                           float* __restrict__ rb) {
  __shared__ float xs[K9];
  __shared__ float red4[4];
  const int s = blockIdx.x, t = threadIdx.x;
  for (int k = t; k < K9; k += 256) xs[k] = xsum[(size_t)s * K9 + k];
  __syncthreads();
  float a = 0.f;
  for (int k = 0; k < K9; ++k) a = fmaf(xs[k], (float)wht[(size_t)k * C + t], a);
  cout[(size_t)s * C + t] = a / 49.f + b[t];
  if (wb) {
    float p = 0.f;
    for (int j = 0; j < 9; ++j) p = fmaf(xs[t + 256 * j], (float)wb[t + 256 * j], p);
    const float tot = block_sum(p, red4);
    if (t == 0) rb[s] = tot / 49.f + bb[0];
  }
}

struct TailFwd { float v0, xhat, rstd, v1, nrm, v2; };

// the class's processed code from its raw code, thread = channel (normalize_code, code_generator.py:832-843)
__device__ __forceinline__ TailFwd tail_forward(float v0, int post_norm, int l2_norm, float ga, float be, float* red4) {
  TailFwd f;
  f.v0 = v0; f.xhat = 0.f; f.rstd = 1.f; f.v1 = v0; f.nrm = 1.f;
  if (post_norm) {
    const float mean = group8_sum(v0) / 8.f;
    const float d = v0 - mean;
    f.rstd = 1.0f / sqrtf(group8_sum(d * d) / 8.f + 1e-5f);
    f.xhat = d * f.rstd;
    f.v1 = f.xhat * ga + be;
  }
  f.v2 = f.v1;
  if (l2_norm) {
    f.nrm = fmaxf(sqrtf(block_sum(f.v1 * f.v1, red4)), 1e-12f);
    f.v2 = f.v1 / f.nrm;
  }
  return f;
}

// one block per class
__global__ __launch_bounds__(256) void cgt_tail_fwd_kernel(const float* __restrict__ cs, const float* __restrict__ rb, const int2* __restrict__ seg,
                                                           CgtCfg cfg, const float* __restrict__ pg, const float* __restrict__ pb,
                                                           const float* __restrict__ conv_scale, const float* __restrict__ bias_scale,
                                                           float* __restrict__ code_raw, float* __restrict__ bias_raw, float* __restrict__ codes) {
  __shared__ float red4[4];
  const int j = blockIdx.x, c = threadIdx.x, s0 = seg[j].x, S = seg[j].y;
  float a = 0.f;
  for (int s = 0; s < S; ++s) a += cs[(size_t)(s0 + s) * C + c];
  const float v0 = a / (float)S;
  code_raw[(size_t)j * C + c] = v0;
  const TailFwd f = tail_forward(v0, cfg.post_norm, cfg.l2_norm, cfg.post_norm ? pg[c] : 1.f, cfg.post_norm ? pb[c] : 0.f, red4);
  codes[(size_t)j * (C + 1) + c] = f.v2 * (conv_scale ? conv_scale[0] : 1.f);
  if (c == 0) {
    float br = 0.f;
    if (cfg.has_bias) {
      for (int s = 0; s < S; ++s) br += rb[s0 + s];
      br = br / (float)S;
    }
    bias_raw[j] = br;
    codes[(size_t)j * (C + 1) + C] = br * (bias_scale ? bias_scale[0] : 1.f) + cfg.prior;
  }
}

// one block per class: tpg / tpb [n_seg][256], tpcs / tpbs [n_seg] are the class's terms of d post_norm.{weight, bias}, d conv_scale, d bias_scale
__global__ __launch_bounds__(256) void cgt_tail_bwd_kernel(const float* __restrict__ code_raw, const float* __restrict__ bias_raw,
                                                           const int2* __restrict__ seg, CgtCfg cfg, const float* __restrict__ pg,
                                                           const float* __restrict__ pb, const float* __restrict__ conv_scale,
                                                           const float* __restrict__ bias_scale, const float* __restrict__ gcodes,
                                                           float* __restrict__ dcode_raw, float* __restrict__ dbias_raw, float* __restrict__ tpg,
                                                           float* __restrict__ tpb, float* __restrict__ tpcs, float* __restrict__ tpbs,
                                                           float* __restrict__ dc, float* __restrict__ drb) {
  __shared__ float red4[4];
  const int j = blockIdx.x, c = threadIdx.x, s0 = seg[j].x, S = seg[j].y;
  const float ga = cfg.post_norm ? pg[c] : 1.f;
  const TailFwd f = tail_forward(code_raw[(size_t)j * C + c], cfg.post_norm, cfg.l2_norm, ga, cfg.post_norm ? pb[c] : 0.f, red4);
  const float g = gcodes[(size_t)j * (C + 1) + c];
  const float dcs = block_sum(g * f.v2, red4);
  const float dv2 = g * (conv_scale ? conv_scale[0] : 1.f);
  float dv1 = dv2;
  if (cfg.l2_norm) {
    const float dot = block_sum(dv2 * f.v2, red4);
    dv1 = (dv2 - f.v2 * dot) / f.nrm;
  }
  float dv0 = dv1;
  if (cfg.post_norm) {
    tpg[(size_t)j * C + c] = dv1 * f.xhat;
    tpb[(size_t)j * C + c] = dv1;
    const float dxh = dv1 * ga;
    const float m1 = group8_sum(dxh) / 8.f, m2 = group8_sum(dxh * f.xhat) / 8.f;
    dv0 = f.rstd * (dxh - m1 - f.xhat * m2);
  }
  dcode_raw[(size_t)j * C + c] = dv0;
  const float per = dv0 / (float)S;
  for (int s = 0; s < S; ++s) dc[(size_t)(s0 + s) * C + c] = per;
  if (c == 0) {
    tpcs[j] = dcs;
    float db = 0.f, dbs = 0.f;
    if (cfg.has_bias) {
      const float gb = gcodes[(size_t)j * (C + 1) + C];
      dbs = gb * bias_raw[j];
      db = gb * (bias_scale ? bias_scale[0] : 1.f);
    }
    tpbs[j] = dbs;
    dbias_raw[j] = db;
    const float pb1 = db / (float)S;
    for (int s = 0; s < S; ++s) drb[s0 + s] = pb1;
  }
}

// out[c] = sum of in[i * ld + c], i = 0 .. n - 1 in that order
__global__ __launch_bounds__(256) void cgt_colsum_kernel(const float* __restrict__ in, int n, int ld, int ncols, float* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= ncols) return;
  float a = 0.f;
  for (int i = 0; i < n; ++i) a += in[(size_t)i * ld + c];
  out[c] = a;
}

// grad (cout, 256, 3, 3): d W[co][k] = sum_s dc[s * cout + co] Xsum[s][k] / 49 in ascending s; a block holds one co
__global__ __launch_bounds__(256) void cgt_head_wgrad_kernel(const float* __restrict__ dc, int cout, const float* __restrict__ xsum, int M,
                                                             float* __restrict__ grad) {
  const int i = blockIdx.x * 256 + threadIdx.x;  // cout * 2304 threads, 2304 = 9 * 256
  const int co = i / K9, k = i - co * K9, tap = k >> 8, ci = k & 255;
  float a = 0.f;
  for (int s = 0; s < M; ++s) a = fmaf(dc[(size_t)s * cout + co], xsum[(size_t)s * K9 + k], a);
  grad[w3x3_torch(co, tap, ci)] = a / 49.f;
}

// d Xsum[s][k] = (sum_co dc[s][co] bf16(W_cls)[co][k] + drb[s] bf16(W_bias)[k]) / 49; grid (9, M)
__global__ __launch_bounds__(256) void cgt_dxsum_kernel(const float* __restrict__ dc, const bf16_t* __restrict__ wh, const float* __restrict__ drb,
                                                        const bf16_t* __restrict__ wb, float* __restrict__ dxsum) {
  __shared__ float g[C];
  const int s = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
  g[threadIdx.x] = dc[(size_t)s * C + threadIdx.x];
  __syncthreads();
  float a = 0.f;
  for (int co = 0; co < C; ++co) a = fmaf(g[co], (float)wh[(size_t)co * K9 + k], a);
  if (wb) a = fmaf(drb[s], (float)wb[k], a);
  dxsum[(size_t)s * K9 + k] = a / 49.f;
}

// d x_L[s][q][ci] = sum of d Xsum[s][tap][ci] over the taps whose box holds q (ascending tap)
__global__ __launch_bounds__(256) void cgt_scatter_kernel(const float* __restrict__ dxsum, float* __restrict__ dx) {
  const int s = blockIdx.x, c = threadIdx.x;
  float d[9];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) d[tap] = dxsum[(size_t)s * K9 + tap * C + c];
#pragma unroll
  for (int qy = 0; qy < 7; ++qy)
#pragma unroll
    for (int qx = 0; qx < 7; ++qx) {
      float a = 0.f;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int ky = tap / 3, kx = tap - 3 * ky;
        if ((unsigned)(qy - ky + 1) < 7u && (unsigned)(qx - kx + 1) < 7u) a += d[tap];
      }
      dx[((size_t)s * NPOS + qy * 7 + qx) * C + c] = a;
    }
}

// one block per shot, thread = channel: dy and the shot's terms gsg / gsb / gsd [M][256] of d gamma, d beta, d (conv bias)
__global__ __launch_bounds__(256) void cgt_gn_bwd_kernel(const float* __restrict__ dxn, const bf16_t* __restrict__ xn, const float* __restrict__ y,
                                                         const float2* __restrict__ stats, const float* __restrict__ gamma, float* __restrict__ dy,
                                                         float* __restrict__ gsg, float* __restrict__ gsb, float* __restrict__ gsd) {
  const int s = blockIdx.x, c = threadIdx.x;
  const size_t base = (size_t)s * NPOS * C + c;
  const float2 st = stats[s * 32 + (c >> 3)];
  const float ga = gamma[c];
  float g[NPOS], xh[NPOS];
  float sg = 0.f, sgx = 0.f;
#pragma unroll
  for (int p = 0; p < NPOS; ++p) {
    const size_t o = base + (size_t)p * C;
    g[p] = (float)xn[o] > 0.f ? dxn[o] : 0.f;
    xh[p] = (y[o] - st.x) * st.y;
    sg += g[p];
    sgx += g[p] * xh[p];
  }
  gsg[(size_t)s * C + c] = sgx;
  gsb[(size_t)s * C + c] = sg;
  const float m1 = group8_sum(ga * sg) / 392.f, m2 = group8_sum(ga * sgx) / 392.f;
  float sd = 0.f;
#pragma unroll
  for (int p = 0; p < NPOS; ++p) {
    const float d = st.y * (g[p] * ga - m1 - xh[p] * m2);
    dy[base + (size_t)p * C] = d;
    sd += d;
  }
  gsd[(size_t)s * C + c] = sd;
}

// part[unit][co][tap][ci] = sum over the unit's rows of bf16(dy)[row][co] x[row + tap][ci].  Grid (36, blocks): blockIdx.x = 4 tap + co
// quarter; a block walks units blockIdx.y, + gridDim.y, ..; wave w owns the input channels [64 w, 64 w + 64).  Per K step 32 rows of both
// operands go to LDS transposed ([channel][row], 80-byte pitch), which is the order the MFMA fragments want
__global__ __launch_bounds__(256) void cgt_wgrad_kernel(const float* __restrict__ dy, const bf16_t* __restrict__ x, const int* __restrict__ shot_map,
                                                        int M, int n_units, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) bf16_t sdy[64][40];
  __shared__ __attribute__((aligned(16))) bf16_t sx[C][40];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lq = lane >> 4;
  const int tap = blockIdx.x >> 2, co0 = (blockIdx.x & 3) * 64, off = tap_off(tap);
  const int j = tid >> 3, t8 = tid & 7;  // staging: row j of the step, eighth t8 of its channels
  for (int unit = blockIdx.y; unit < n_units; unit += gridDim.y) {
    const int r0 = unit * CGT_UNIT_SHOTS * NPOS, r1 = min(M, (unit + 1) * CGT_UNIT_SHOTS) * NPOS;
    f32x4v acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int n = 0; n < 4; ++n) acc[i][n] = f32x4v{0.f, 0.f, 0.f, 0.f};
    for (int rs = r0; rs < r1; rs += 32) {
      const int r = rs + j;
      float dv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) dv[e] = 0.f;
      long srow = -1;
      if (r < r1) {
        load8<float>(dy + (size_t)r * C + co0 + t8 * 8, dv);
        const int s = r / NPOS, p = r - s * NPOS, py = p / 7, px = p - 7 * py;
        if (tap_ok(py, px, tap)) srow = (long)(shot_map ? shot_map[s] : s) * NPOS + p + off;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) sdy[t8 * 8 + e][j] = (bf16_t)dv[e];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        bf16x8 v;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (bf16_t)0.f;
        if (srow >= 0) v = *reinterpret_cast<const bf16x8*>(x + (size_t)srow * C + t8 * 32 + q * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) sx[t8 * 32 + q * 8 + e][j] = v[e];
      }
      __syncthreads();
      bf16x8 fa[4], fb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[i] = *reinterpret_cast<const bf16x8*>(&sdy[16 * i + l15][lq * 8]);
#pragma unroll
      for (int n = 0; n < 4; ++n) fb[n] = *reinterpret_cast<const bf16x8*>(&sx[wave * 64 + 16 * n + l15][lq * 8]);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[i][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[n], acc[i][n], 0, 0, 0);
      __syncthreads();
    }
    // accumulator layout: co = co0 + 16 i + 4 lq + e, ci = 64 wave + 16 n + l15
    float* pp = part + (size_t)unit * C * K9;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          pp[(size_t)(co0 + 16 * i + 4 * lq + e) * K9 + tap * C + wave * 64 + 16 * n + l15] = acc[i][n][e];
  }
}

// the sink of the tree's final kernel: element i of the summed partial [co][tap][ci] -> grad (co, ci, ky, kx)
struct CgtWgradSink {
  float* grad;
  __device__ void operator()(int i, float s) const {
    const int co = i / K9, k = i - co * K9, tap = k >> 8, ci = k & 255;
    grad[w3x3_torch(co, tap, ci)] = s;
  }
};

__global__ __launch_bounds__(256) void cgt_bf16_to_f32_kernel(const bf16_t* __restrict__ in, size_t n, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (float)in[i];
}

int cgt_block_cap() { return block_cap("SYLPH_CODEGEN_TRAIN_BLOCKS", CGT_MAX_BLOCKS); }

template <typename TIn>
void conv(const TIn* in, const int* shot_map, const bf16_t* wp, const float* bias, float* out, int rows, hipStream_t s) {
  const int tiles = (rows + 31) / 32, cap = cgt_block_cap();
  hipLaunchKernelGGL(cgt_conv_kernel<TIn>, dim3(tiles < cap ? tiles : cap), dim3(256), 0, s, in, shot_map, wp, bias, out, rows);
}

void colsum(const float* in, int n, int ld, int ncols, float* out, hipStream_t s) {
  hipLaunchKernelGGL(cgt_colsum_kernel, dim3((ncols + 255) / 256), dim3(256), 0, s, in, n, ld, ncols, out);
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

void cgt_param_layout(const CgtCfg& cfg, CgtParams* p) {
  long o = 0;
  for (int i = 0; i < CGT_MAX_TOWER; ++i) p->tw[i] = p->tb[i] = p->tg[i] = p->tbe[i] = -1;
  for (int i = 0; i < cfg.L; ++i) {
    p->tw[i] = o; o += (long)C * K9;
    p->tb[i] = o; o += C;
    p->tg[i] = o; o += C;
    p->tbe[i] = o; o += C;
  }
  p->cw = o; o += (long)C * K9;
  p->cb = o; o += C;
  p->bw = p->bb = p->pg = p->pb = p->cs = p->bs = -1;
  if (cfg.has_bias) { p->bw = o; o += K9; p->bb = o; o += 1; }
  if (cfg.post_norm) { p->pg = o; o += C; p->pb = o; o += C; }
  if (cfg.has_conv_scale) { p->cs = o; o += 1; }
  if (cfg.has_bias) { p->bs = o; o += 1; }
  p->total = o;
}

void cgt_workspace(const CgtCfg& cfg, int M, int n_seg, CgtWs* w) {
  const size_t R = (size_t)M * NPOS;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o = align256(o + bytes); return at; };
  w->idx = take((size_t)M * 4);
  w->seg = take((size_t)n_seg * 8);
  for (int i = 0; i < cfg.L; ++i) {
    w->wf[i] = take((size_t)C * K9 * 2);
    w->wd[i] = take((size_t)C * K9 * 2);
    w->y[i] = take(R * C * 4);
    w->st[i] = take((size_t)M * 32 * 8);
    w->x[i] = take(R * C * 2);
  }
  w->wh = take((size_t)C * K9 * 2);
  w->wht = take((size_t)C * K9 * 2);
  w->wb = take((size_t)K9 * 2);
  w->xsum = take((size_t)M * K9 * 4);
  w->c = take((size_t)M * C * 4);
  w->rb = take((size_t)M * 4);
  w->code_raw = take((size_t)n_seg * C * 4);
  w->bias_raw = take((size_t)n_seg * 4);
  w->dcode_raw = take((size_t)n_seg * C * 4);
  w->dbias_raw = take((size_t)n_seg * 4);
  w->tpg = take((size_t)n_seg * C * 4);
  w->tpb = take((size_t)n_seg * C * 4);
  w->tpcs = take((size_t)n_seg * 4);
  w->tpbs = take((size_t)n_seg * 4);
  w->dc = take((size_t)M * C * 4);
  w->drb = take((size_t)M * 4);
  w->dxsum = take((size_t)M * K9 * 4);
  w->dxa = take(cfg.L ? R * C * 4 : 0);
  w->dya = take(cfg.L ? R * C * 4 : 0);
  w->gsg = take((size_t)M * C * 4);
  w->gsb = take((size_t)M * C * 4);
  w->gsd = take((size_t)M * C * 4);
  w->units = (M + CGT_UNIT_SHOTS - 1) / CGT_UNIT_SHOTS;
  const PartialTree tree = partial_tree(cfg.L ? w->units : 0, CGT_FANIN);  // without a tower no weight gradient goes through the tree
  w->passes = tree.passes;
  w->part = take(tree.planes * C * K9 * 4);
  w->total = o;
}

// debug_out: forward stages, then backward stages, every one fp32:
//   per layer i < L: y_i [R][256] | (mean, rstd) [M][32][2] | x_{i+1} [R][256];  Xsum [M][2304] | c [M][256] | rb [M] | code_raw [n_seg][256] | bias_raw [n_seg]
//   d code_raw [n_seg][256] | d bias_raw [n_seg] | d c [M][256] | d rb [M] | L >= 1: d Xsum [M][2304] | d x_L [R][256] | for i = L - 1 .. 0: d y_i [R][256] | i >= 1: d x_i [R][256]
size_t cgt_debug_floats(const CgtCfg& cfg, int M, int n_seg) {
  const size_t R = (size_t)M * NPOS, L = (size_t)cfg.L;
  size_t n = L * (2 * R * C + (size_t)M * 64) + (size_t)M * K9 + (size_t)M * C + M + (size_t)n_seg * C + n_seg;
  n += (size_t)n_seg * C + n_seg + (size_t)M * C + M;
  if (L) n += (size_t)M * K9 + R * C + L * R * C + (L - 1) * R * C;
  return n;
}

int launch_cgt_forward(const CgtCfg& cfg, const float* params, const void* rows, int M, int n_seg, char* ws, float* codes_out, hipStream_t s) {
  if (M < 1 || n_seg < 1 || cfg.L < 0 || cfg.L > CGT_MAX_TOWER) return -1;
  CgtParams P;
  CgtWs W;
  cgt_param_layout(cfg, &P);
  cgt_workspace(cfg, M, n_seg, &W);
  const int R = M * NPOS;
  const int* idx = reinterpret_cast<const int*>(ws + W.idx);
  const int2* seg = reinterpret_cast<const int2*>(ws + W.seg);
  const bf16_t* x = static_cast<const bf16_t*>(rows);
  const int* map = idx;
  for (int i = 0; i < cfg.L; ++i) {
    bf16_t* wf = reinterpret_cast<bf16_t*>(ws + W.wf[i]);
    hipLaunchKernelGGL(cgt_pack_kernel, dim3(C * K9 / 256), dim3(256), 0, s, params + P.tw[i], C, wf, reinterpret_cast<bf16_t*>(ws + W.wd[i]),
                       (bf16_t*)nullptr);
    float* y = reinterpret_cast<float*>(ws + W.y[i]);
    conv<bf16_t>(x, map, wf, params + P.tb[i], y, R, s);
    bf16_t* xn = reinterpret_cast<bf16_t*>(ws + W.x[i]);
    hipLaunchKernelGGL(cgt_gn_fwd_kernel, dim3(M), dim3(256), 0, s, y, params + P.tg[i], params + P.tbe[i], reinterpret_cast<float2*>(ws + W.st[i]), xn);
    x = xn;
    map = nullptr;
  }
  bf16_t* wht = reinterpret_cast<bf16_t*>(ws + W.wht);
  bf16_t* wb = cfg.has_bias ? reinterpret_cast<bf16_t*>(ws + W.wb) : nullptr;
  hipLaunchKernelGGL(cgt_pack_kernel, dim3(C * K9 / 256), dim3(256), 0, s, params + P.cw, C, reinterpret_cast<bf16_t*>(ws + W.wh), (bf16_t*)nullptr, wht);
  if (wb) hipLaunchKernelGGL(cgt_pack_kernel, dim3(K9 / 256), dim3(256), 0, s, params + P.bw, 1, wb, (bf16_t*)nullptr, (bf16_t*)nullptr);
  float* xsum = reinterpret_cast<float*>(ws + W.xsum);
  hipLaunchKernelGGL(cgt_xsum_kernel, dim3(M), dim3(256), 0, s, x, map, xsum);
  float* cs = reinterpret_cast<float*>(ws + W.c);
  float* rb = reinterpret_cast<float*>(ws + W.rb);
  hipLaunchKernelGGL(cgt_head_fwd_kernel, dim3(M), dim3(256), 0, s, xsum, wht, params + P.cb, wb, wb ? params + P.bb : nullptr, cs, rb);
  hipLaunchKernelGGL(cgt_tail_fwd_kernel, dim3(n_seg), dim3(256), 0, s, cs, rb, seg, cfg, cfg.post_norm ? params + P.pg : nullptr,
                     cfg.post_norm ? params + P.pb : nullptr, P.cs >= 0 ? params + P.cs : nullptr, P.bs >= 0 ? params + P.bs : nullptr,
                     reinterpret_cast<float*>(ws + W.code_raw), reinterpret_cast<float*>(ws + W.bias_raw), codes_out);
  return (int)hipGetLastError();
}

int launch_cgt_backward(const CgtCfg& cfg, const float* params, const void* rows, int M, int n_seg, char* ws, const float* grad_codes,
                        float* grad_out, float* debug_out, hipStream_t s) {
  if (M < 1 || n_seg < 1 || cfg.L < 0 || cfg.L > CGT_MAX_TOWER) return -1;
  CgtParams P;
  CgtWs W;
  cgt_param_layout(cfg, &P);
  cgt_workspace(cfg, M, n_seg, &W);
  const size_t R = (size_t)M * NPOS;
  const int L = cfg.L;
  const int* idx = reinterpret_cast<const int*>(ws + W.idx);
  const int2* seg = reinterpret_cast<const int2*>(ws + W.seg);
  auto F = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
  auto H = [&](size_t off) { return reinterpret_cast<bf16_t*>(ws + off); };
  float* dbg = debug_out;
  auto put = [&](const float* src, size_t n) {
    if (!dbg) return;
    (void)hipMemcpyAsync(dbg, src, n * 4, hipMemcpyDeviceToDevice, s);
    dbg += n;
  };
  auto put_h = [&](const bf16_t* src, size_t n) {
    if (!dbg) return;
    hipLaunchKernelGGL(cgt_bf16_to_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, n, dbg);
    dbg += n;
  };
  for (int i = 0; i < L; ++i) {
    put(F(W.y[i]), R * C);
    put(F(W.st[i]), (size_t)M * 64);
    put_h(H(W.x[i]), R * C);
  }
  put(F(W.xsum), (size_t)M * K9);
  put(F(W.c), (size_t)M * C);
  put(F(W.rb), M);
  put(F(W.code_raw), (size_t)n_seg * C);
  put(F(W.bias_raw), n_seg);

  (void)hipMemsetAsync(grad_out, 0, (size_t)P.total * 4, s);
  float *dc = F(W.dc), *drb = F(W.drb), *xsum = F(W.xsum);
  hipLaunchKernelGGL(cgt_tail_bwd_kernel, dim3(n_seg), dim3(256), 0, s, F(W.code_raw), F(W.bias_raw), seg, cfg, cfg.post_norm ? params + P.pg : nullptr,
                     cfg.post_norm ? params + P.pb : nullptr, P.cs >= 0 ? params + P.cs : nullptr, P.bs >= 0 ? params + P.bs : nullptr, grad_codes,
                     F(W.dcode_raw), F(W.dbias_raw), F(W.tpg), F(W.tpb), F(W.tpcs), F(W.tpbs), dc, drb);
  if (cfg.post_norm) {
    colsum(F(W.tpg), n_seg, C, C, grad_out + P.pg, s);
    colsum(F(W.tpb), n_seg, C, C, grad_out + P.pb, s);
  }
  if (P.cs >= 0) colsum(F(W.tpcs), n_seg, 1, 1, grad_out + P.cs, s);
  if (P.bs >= 0) colsum(F(W.tpbs), n_seg, 1, 1, grad_out + P.bs, s);
  put(F(W.dcode_raw), (size_t)n_seg * C);
  put(F(W.dbias_raw), n_seg);
  put(dc, (size_t)M * C);
  put(drb, M);
  // the heads
  hipLaunchKernelGGL(cgt_head_wgrad_kernel, dim3(C * K9 / 256), dim3(256), 0, s, dc, C, xsum, M, grad_out + P.cw);
  colsum(dc, M, C, C, grad_out + P.cb, s);
  if (cfg.has_bias) {
    hipLaunchKernelGGL(cgt_head_wgrad_kernel, dim3(K9 / 256), dim3(256), 0, s, drb, 1, xsum, M, grad_out + P.bw);
    colsum(drb, M, 1, 1, grad_out + P.bb, s);
  }
  if (L > 0) {
    float *dxa = F(W.dxa), *dya = F(W.dya), *part = F(W.part);
    hipLaunchKernelGGL(cgt_dxsum_kernel, dim3(K9 / 256, M), dim3(256), 0, s, dc, H(W.wh), drb, cfg.has_bias ? H(W.wb) : nullptr, F(W.dxsum));
    hipLaunchKernelGGL(cgt_scatter_kernel, dim3(M), dim3(256), 0, s, F(W.dxsum), dxa);
    put(F(W.dxsum), (size_t)M * K9);
    put(dxa, R * C);
    const int cap = cgt_block_cap();
    for (int i = L - 1; i >= 0; --i) {
      hipLaunchKernelGGL(cgt_gn_bwd_kernel, dim3(M), dim3(256), 0, s, dxa, H(W.x[i]), F(W.y[i]), reinterpret_cast<const float2*>(ws + W.st[i]),
                         params + P.tg[i], dya, F(W.gsg), F(W.gsb), F(W.gsd));
      colsum(F(W.gsg), M, C, C, grad_out + P.tg[i], s);
      colsum(F(W.gsb), M, C, C, grad_out + P.tbe[i], s);
      colsum(F(W.gsd), M, C, C, grad_out + P.tb[i], s);
      put(dya, R * C);
      const int u = W.units;
      const bf16_t* xin = i > 0 ? H(W.x[i - 1]) : static_cast<const bf16_t*>(rows);
      hipLaunchKernelGGL(cgt_wgrad_kernel, dim3(36, u < cap ? u : cap), dim3(256), 0, s, dya, xin, i > 0 ? (const int*)nullptr : idx, M, u, part);
      partial_final(partial_sum_passes(part, u, C * K9, CGT_FANIN, s), C * K9, C * K9, CgtWgradSink{grad_out + P.tw[i]}, s);
      if (i > 0) {
        conv<float>(dya, nullptr, H(W.wd[i]), nullptr, dxa, (int)R, s);
        put(dxa, R * C);
      }
    }
  }
  return (int)hipGetLastError();
}

}  // namespace sylph
