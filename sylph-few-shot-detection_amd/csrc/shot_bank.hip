// Shot bank: the support path cut at its per-shot stage.  shot_pool_kernel writes what codegen_tail_kernel (codegen.hip) computes from
// ONE shot alone -- the pooled cls_conv map, the pooled bias term, the pooled shot-weight logit, the pooled class-scale term -- as one row
// per ROI; shot_combine_kernel forms the code of any list of such rows, gathered through an index list, with the tail's own
// combination: the strided softmax (or 1/S), then code += w[s] * v in list order.  Every operation and every order of additions is
// the tail's, and this unit is compiled with -ffp-contract=off like codegen.hip, so pool + combine gives the tail's bits.
// For the ROIEncoder a row is the shot's token after the last encoder layer and the combination is mean_tokens_kernel's
// (roi_encoder.hip: additions in list order, one division).
//
// Reference arithmetic followed (paths relative to /root/reference), as in codegen.hip / roi_encoder.hip:
//   sylph/modeling/code_generator/code_generator.py:954-967   conv / bias features, BIAS_L2_NORM (per shot)
//   sylph/modeling/code_generator/utils.py:51-67              GlobalAdaptiveAvgPool2d (per shot)
//   sylph/modeling/code_generator/code_generator.py:766-829   shot weights, compute_code (per class)
//   sylph/modeling/code_generator/roi_encoder.py:184-196      the class token: mean over the shots
#include "common.h"
#include "kernels.h"

namespace sylph {

// Row r of rows[R][row_ld] from conv_out [R*npos][conv_ld] and aux_out [R*npos][aux_ld] (channels ib / iw / is, -1 = absent):
//   [0, C k^2)   sum / npos over p = 0 .. npos-1 in that order (k = 1), or sum / 9 over the 3x3 bin [0,3) [2,5) [4,7) of each axis in
//                (dy, dx) order at (c * 3 + ky) * 3 + kx (k = 3, npos == 49)
//   C k^2        bias term: the 64-lane xor tree over the positions (of v / max(||v||, 1e-12) with BIAS_L2_NORM), / npos
//   C k^2 + 1    shot-weight logit: sequential sum over p, / npos
//   C k^2 + 2    class-scale term: xor tree, / npos
//   C k^2 + 3    0 (rows stay 16-byte aligned)
// One block of 256 threads per ROI.
__global__ __launch_bounds__(256) void shot_pool_kernel(const float* __restrict__ conv_out, int conv_ld, const float* __restrict__ aux_out,
                                                        int aux_ld, int ib, int iw, int is, int npos, int C, int ksize, int bias_l2_norm,
                                                        float* __restrict__ rows, int row_ld) {
  conv_out += (size_t)blockIdx.x * npos * conv_ld;
  aux_out += (size_t)blockIdx.x * npos * aux_ld;
  float* row = rows + (size_t)blockIdx.x * row_ld;
  if (ksize == 3) {
    for (int i = threadIdx.x; i < C * 9; i += blockDim.x) {  // npos == 49
      const int c = i / 9, t = i - c * 9, ky = t / 3, kx = t - ky * 3;
      const int y0 = (ky * 7) / 3, x0 = (kx * 7) / 3;
      float sum = 0.f;
      for (int dy = 0; dy < 3; ++dy)
        for (int dx = 0; dx < 3; ++dx) sum += conv_out[(size_t)((y0 + dy) * 7 + x0 + dx) * conv_ld + c];
      row[i] = sum / 9.f;
    }
  } else {
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
      float sum = 0.f;
      for (int p = 0; p < npos; ++p) sum += conv_out[(size_t)p * conv_ld + c];
      row[c] = sum / (float)npos;
    }
  }
  if (threadIdx.x < 64) {  // one wave: the three 1-channel heads
    const int lane = threadIdx.x;
    float bias = 0.f, wn = 0.f, lg = 0.f;
    if (ib >= 0) {
      const float v = lane < npos ? aux_out[(size_t)lane * aux_ld + ib] : 0.f;  // npos <= 64
      float nrm = 1.f;
      if (bias_l2_norm) {
        float sq = v * v;
        for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
        nrm = fmaxf(sqrtf(sq), 1e-12f);
      }
      float t = v / nrm;
      for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
      bias = t / (float)npos;
    }
    if (is >= 0) {
      float t = lane < npos ? aux_out[(size_t)lane * aux_ld + is] : 0.f;
      for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
      wn = t / (float)npos;
    }
    if (iw >= 0 && lane == 0) {
      float sum = 0.f;
      for (int p = 0; p < npos; ++p) sum += aux_out[(size_t)p * aux_ld + iw];
      lg = sum / (float)npos;
    }
    if (lane == 0) {
      float* tail = row + C * ksize * ksize;
      tail[0] = bias; tail[1] = lg; tail[2] = wn; tail[3] = 0.f;
    }
  }
}

int launch_shot_pool(const float* conv_out, int conv_ld, const float* aux_out, int aux_ld, int ib, int iw, int is, int R, int npos, int C,
                     int ksize, int bias_l2_norm, float* rows, int row_ld, hipStream_t s) {
  if (npos > 64 || R < 1 || (ksize != 1 && !(ksize == 3 && npos == 49)) || row_ld < C * ksize * ksize + 4) return -1;
  hipLaunchKernelGGL(shot_pool_kernel, dim3(R), dim3(256), 0, s, conv_out, conv_ld, aux_out, aux_ld, ib, iw, is, npos, C, ksize, bias_l2_norm,
                     rows, row_ld);
  return (int)hipGetLastError();
}

// ROIEncoder rows: the shot's 256-float token, then four zeros (the CodeGenerator's 1x1 row width)
__global__ __launch_bounds__(256) void shot_token_rows_kernel(const float* __restrict__ tok, float* __restrict__ rows, int row_ld) {
  const int t = threadIdx.x;
  float* row = rows + (size_t)blockIdx.x * row_ld;
  row[t] = tok[(size_t)blockIdx.x * 256 + t];
  if (t < row_ld - 256) row[256 + t] = 0.f;
}

int launch_shot_token_rows(const float* tok, int R, float* rows, int row_ld, hipStream_t s) {
  if (R < 1 || row_ld < 256 || row_ld > 512) return -1;
  hipLaunchKernelGGL(shot_token_rows_kernel, dim3(R), dim3(256), 0, s, tok, rows, row_ld);
  return (int)hipGetLastError();
}

// code_out[j][n + 1] (+ wnorm_out[j]) from the rows idx[seg[j].x + i], i < seg[j].y, of a bank rows[.][row_ld] whose rows are
// shot_pool_kernel's (n = C k^2 code values, then bias term | logit | scale term | pad).  One block per segment; what
// codegen_tail_kernel does after its per-shot sums, on the stored values: lane l of the first wave owns shots l, l + 64, ... of the
// softmax (has_w; else 1 / S), the weights sit in dynamic LDS, and every output accumulates code += w[s] * v for s = 0 .. S-1.
// Threads walk a row contiguously (VEC: four floats per thread; the host asks for it when rows are 16-byte aligned and wide enough
// to keep the block busy), so each shot is one coalesced row read.  An index may repeat.
template <bool VEC>
__global__ __launch_bounds__(256) void shot_combine_kernel(const float* __restrict__ rows, int row_ld, const int* __restrict__ idx,
                                                           const int2* __restrict__ seg, int n, int has_b, int has_w, int has_s,
                                                           float* __restrict__ code_out, float* __restrict__ wnorm_out) {
  extern __shared__ float wsh[];  // per-shot weights: max(64, longest segment) floats
  const int S = seg[blockIdx.x].y;
  idx += seg[blockIdx.x].x;
  code_out += (size_t)blockIdx.x * (n + 1);
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    if (has_w) {
      float mx = -INFINITY;
      for (int i = lane; i < S; i += 64) {
        const float lg = rows[(size_t)idx[i] * row_ld + n + 1];
        wsh[i] = lg;
        mx = fmaxf(mx, lg);
      }
      for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
      float den = 0.f;
      for (int i = lane; i < S; i += 64) {
        const float e = expf(wsh[i] - mx);
        wsh[i] = e;
        den += e;
      }
      for (int o = 32; o > 0; o >>= 1) den += __shfl_xor(den, o);
      for (int i = lane; i < S; i += 64) wsh[i] = wsh[i] / den;
    } else {
      for (int i = lane; i < S; i += 64) wsh[i] = 1.0f / (float)S;
    }
  }
  __syncthreads();
  if (VEC) {  // n % 4 == 0, rows 16-byte aligned; the code row itself starts at a multiple of n + 1 floats: scalar stores
    for (int i = threadIdx.x * 4; i < n; i += blockDim.x * 4) {
      float c0 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f;
      for (int s = 0; s < S; ++s) {
        const float4 v = *reinterpret_cast<const float4*>(rows + (size_t)idx[s] * row_ld + i);
        const float w = wsh[s];
        c0 += w * v.x; c1 += w * v.y; c2 += w * v.z; c3 += w * v.w;
      }
      code_out[i] = c0; code_out[i + 1] = c1; code_out[i + 2] = c2; code_out[i + 3] = c3;
    }
  } else {
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      float code = 0.f;
      for (int s = 0; s < S; ++s) code += wsh[s] * rows[(size_t)idx[s] * row_ld + i];
      code_out[i] = code;
    }
  }
  if (threadIdx.x == blockDim.x - 1) {  // the two pooled heads, in shot order like the tail's wave
    float bias = 0.f, wn = 0.f;
    for (int s = 0; s < S; ++s) {
      const float* r = rows + (size_t)idx[s] * row_ld + n;
      if (has_b) bias += wsh[s] * r[0];
      if (has_s) wn += wsh[s] * r[2];
    }
    code_out[n] = bias;
    if (wnorm_out) wnorm_out[blockIdx.x] = wn;
  }
}

int launch_shot_combine(const float* rows, int row_ld, const int* idx_dev, const int2* seg_dev, int n_seg, int max_len, int n, int has_b,
                        int has_w, int has_s, float* code_out, float* wnorm_out, hipStream_t s) {
  if (n_seg < 1 || max_len < 1 || max_len > TAIL_MAX_LEN || n < 1 || row_ld < n + 4) return -1;
  const size_t lds = (size_t)(max_len > 64 ? max_len : 64) * sizeof(float);
  const bool vec = n % 4 == 0 && n / 4 >= 256 && row_ld % 4 == 0 && ((uintptr_t)rows & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(shot_combine_kernel<true>, dim3(n_seg), dim3(256), lds, s, rows, row_ld, idx_dev, seg_dev, n, has_b, has_w, has_s,
                       code_out, has_s ? wnorm_out : nullptr);
  else
    hipLaunchKernelGGL(shot_combine_kernel<false>, dim3(n_seg), dim3(256), lds, s, rows, row_ld, idx_dev, seg_dev, n, has_b, has_w, has_s,
                       code_out, has_s ? wnorm_out : nullptr);
  return (int)hipGetLastError();
}

// mean_tokens_kernel on gathered rows: out[j][t] = (sum over i < seg[j].y, in that order, of rows[idx[seg[j].x + i]][t]) / seg[j].y
__global__ __launch_bounds__(256) void shot_mean_tokens_kernel(const float* __restrict__ rows, int row_ld, const int* __restrict__ idx,
                                                               const int2* __restrict__ seg, float* __restrict__ out) {
  const int t = threadIdx.x, c = blockIdx.x;
  const int S = seg[c].y;
  idx += seg[c].x;
  float a = 0.f;
  for (int s = 0; s < S; ++s) a += rows[(size_t)idx[s] * row_ld + t];
  out[(size_t)c * 256 + t] = a / (float)S;
}

int launch_shot_mean_tokens(const float* rows, int row_ld, const int* idx_dev, const int2* seg_dev, int n_seg, float* out, hipStream_t s) {
  if (n_seg < 1 || row_ld < 256) return -1;
  hipLaunchKernelGGL(shot_mean_tokens_kernel, dim3(n_seg), dim3(256), 0, s, rows, row_ld, idx_dev, seg_dev, out);
  return (int)hipGetLastError();
}

}  // namespace sylph
