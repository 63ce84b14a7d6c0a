// The two direct convolutions of the MobileNetV2 bottom-up path (AdelaiDet adet/modeling/backbone/mobilenet.py, via
// meta_one_stage_detector.py:181,273), gfx950.  Plain vector code, fp32 arithmetic in every storage mode, 16 bytes per lane.
//   dwconv3x3_kernel   depthwise 3x3, pad 1, stride 1 / 2: y = relu6(scale * conv(clamp(x, 0, 6)) + shift).  The clamp on load is the
//                      ReLU6 of the layer in front (the 1x1 expand, whose launch stores bn(conv) without it): 0 and 6 are exact in bf16
//                      and rounding is monotonic, so clamp(round(v)) == round(clamp(v)).
//   mbv2_stem_kernel   features.0: 3x3 stride 2 pad 1, 3 -> 32 + FrozenBN + ReLU6 on the normalised padded batch [B][H][W][4]
// Rows have a pitch of ld >= C elements (the pitch the 1x1 kernels around them store with); channels [C, ld) are neither read nor written.
// Every index that can pass 2^31 is size_t; a thread either owns 8 channels of one in-range output position or returns.
#include "common.h"
#include "kernels.h"

namespace sylph {

__device__ __forceinline__ float relu6f(float v) { return fminf(fmaxf(v, 0.f), 6.f); }

template <typename T>
__global__ void __launch_bounds__(256) dwconv3x3_kernel(DwConvArgs a) {
  const int cg = a.C >> 3;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)a.B * a.Ho * a.Wo * cg) return;
  const int c0 = (int)(idx % cg) * 8;
  size_t pos = idx / cg;
  const int ox = (int)(pos % a.Wo);
  pos /= a.Wo;
  const int oy = (int)(pos % a.Ho), b = (int)(pos / a.Ho);
  const T* xb = (const T*)a.x + (size_t)b * a.H * a.W * a.ld + c0;
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int iy = oy * a.stride - 1 + kh;
    if (iy < 0 || iy >= a.H) continue;
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int ix = ox * a.stride - 1 + kw;
      if (ix < 0 || ix >= a.W) continue;
      float v[8], w[8];
      load8<T>(xb + ((size_t)iy * a.W + ix) * a.ld, v);
      load8<float>(a.w + (size_t)(kh * 3 + kw) * a.C + c0, w);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = fmaf(relu6f(v[i]), w[i], acc[i]);
    }
  }
  float sc[8], sh[8], o[8];
  load8<float>(a.scale + c0, sc);
  load8<float>(a.shift + c0, sh);
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = relu6f(fmaf(acc[i], sc[i], sh[i]));
  store8<T>((T*)a.y + (((size_t)b * a.Ho + oy) * a.Wo + ox) * a.ld + c0, o);
}

int launch_dwconv3x3(DType dt, const DwConvArgs& a, hipStream_t s) {
  if (a.C < 8 || (a.C & 7) || a.ld < a.C || (a.ld & 7) || (a.stride != 1 && a.stride != 2) || a.B < 1 || a.H < 1 || a.W < 1) return -4;
  if (a.Ho != (a.H - 1) / a.stride + 1 || a.Wo != (a.W - 1) / a.stride + 1) return -4;
  const size_t n = (size_t)a.B * a.Ho * a.Wo * (a.C >> 3), blocks = (n + 255) / 256;
  if (blocks > 0x7fffffffu) return -5;
  if (dt == DT_BF16) hipLaunchKernelGGL(dwconv3x3_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(dwconv3x3_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

// x [B][H][W][4] (channel 3 zero), w fp32 [3][3][4][32] (input channel 3 zero), y [B][Ho * Wo][ld], channels [0, C) of every row with
// C >= 32 a multiple of 8: channels >= 32 are the storage padding and are written as zeros.
template <typename T>
__global__ void __launch_bounds__(256) mbv2_stem_kernel(MbStemArgs a) {
  __shared__ float ws[9 * 4 * 32];
  for (int i = threadIdx.x; i < 9 * 4 * 32; i += 256) ws[i] = a.w[i];
  __syncthreads();
  const int cg = a.C >> 3;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)a.B * a.Ho * a.Wo * cg) return;
  const int c0 = (int)(idx % cg) * 8;
  size_t pos = idx / cg;
  const int ox = (int)(pos % a.Wo);
  pos /= a.Wo;
  const int oy = (int)(pos % a.Ho), b = (int)(pos / a.Ho);
  float o[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = 0.f;
  if (c0 < 32) {
    const T* xb = (const T*)a.x + (size_t)b * a.H * a.W * 4;
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int iy = oy * 2 - 1 + kh;
      if (iy < 0 || iy >= a.H) continue;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int ix = ox * 2 - 1 + kw;
        if (ix < 0 || ix >= a.W) continue;
        const T* p = xb + ((size_t)iy * a.W + ix) * 4;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const float v = Cvt<T>::to_f(p[ch]);
          const float* wr = ws + ((kh * 3 + kw) * 4 + ch) * 32 + c0;
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[i] = fmaf(v, wr[i], acc[i]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = relu6f(fmaf(acc[i], a.scale[c0 + i], a.shift[c0 + i]));
  }
  store8<T>((T*)a.y + (((size_t)b * a.Ho + oy) * a.Wo + ox) * a.ld + c0, o);
}

int launch_mbv2_stem(DType dt, const MbStemArgs& a, hipStream_t s) {
  if (a.C < 32 || (a.C & 7) || a.ld < a.C || (a.ld & 7) || a.B < 1 || a.H < 1 || a.W < 1 || a.Ho != (a.H - 1) / 2 + 1 || a.Wo != (a.W - 1) / 2 + 1) return -4;
  const size_t n = (size_t)a.B * a.Ho * a.Wo * (a.C >> 3), blocks = (n + 255) / 256;
  if (blocks > 0x7fffffffu) return -5;
  if (dt == DT_BF16) hipLaunchKernelGGL(mbv2_stem_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(mbv2_stem_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

}  // namespace sylph
