// Grouped 3x3 convolution for gfx950: conv2 of a ResNeXt bottleneck (detectron2 BottleneckBlock with num_groups > 1),
// pad 1, stride 1 or 2, FrozenBN scale / shift and ReLU fused in the epilogue:
//
//   y[b][p][n] = relu( fma( sum_{tap, c < cpg} x[b][in(p, tap)][g(n) cpg + c] W[n][c][tap], scale[n], shift[n] ) ),  g(n) = n / cpg
//
// Activations are NHWC rows [B][H * W][C]; every image is addressed from a 64-bit base, with 32-bit element offsets inside it
// (launch_conv_group refuses an image of 2^31 elements or more).  C is a multiple of 64, cpg (channels per group) a power of two in
// [4, 64].
//
// bf16 (16x16x32 MFMA, fp32 accumulate, bf16 store): a wave owns 64 output positions (four 16-position M tiles) of one 64-channel
// slab; the four waves of a block own four neighbouring slabs of the same positions.  As groups never straddle a slab, a slab's
// outputs read only the slab's inputs.  The slab is cut into windows of KW = max(16, cpg) channels: the outputs of a window read
// only the window's inputs, so a window is a small dense GEMM with K = 9 taps x KW channels (K chunks of 8 channels, tap-major,
// padded to whole MFMAs) and N = KW.  Below 16 channels per group the 16x16 weight block of a window is block-diagonal: 4 or 8
// channels per group waste 75 % / 50 % of those MFMAs, which this memory-bound layer affords.  The weights are the MFMA A operand
// (output channel on the MFMA row), pre-packed in lane order (conv_group_pack), so each lane holds four consecutive output channels
// of one position and stores them as one 8-byte write.  The activations are the B operand: each lane loads its 16-byte chunk of one
// tap straight from global memory (L1 / L2 serve the nine-tap reuse); taps outside the map read as zeros.
//
// fp32 (DT_F32) and split-bf16 (DT_F32S, fp32 storage) run this layer in exact fp32 on the VALU: one thread per (position, four
// output channels), products summed tap-major, channel by channel, with fmaf.
#include <string.h>

#include "common.h"
#include "kernels.h"

namespace sylph {

namespace {

typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

template <int KW>
struct GroupTile {
  static constexpr int CT = KW / 8;              // 8-channel K chunks per tap
  static constexpr int NS = (9 * CT + 3) / 4;    // 16x16x32 MFMAs per window (4 chunks each, the tail padded with zeros)
  static constexpr int NW = 64 / KW;             // windows per 64-channel slab
  static constexpr int NTW = KW / 16;            // 16-channel N tiles per window
};

template <int KW>
__global__ __launch_bounds__(256) void conv_group_bf16_kernel(GroupConvArgs a) {
  typedef GroupTile<KW> T;
  const int lane = threadIdx.x & 63, slab = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (slab >= a.C / 64) return;
  const int P = a.Ho * a.Wo, p0 = blockIdx.x * 64, r = lane & 15, h = lane >> 4;
  const bf16_t* x = reinterpret_cast<const bf16_t*>(a.x) + (size_t)blockIdx.z * a.Hin * a.Win * a.C + slab * 64;
  bf16_t* y = reinterpret_cast<bf16_t*>(a.y) + (size_t)blockIdx.z * P * a.C + slab * 64;
  const bf16x8* wt = reinterpret_cast<const bf16x8*>(a.wt) + (size_t)slab * T::NW * T::NS * T::NTW * 64 + lane;
  int iy0[4], ix0[4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const int p = p0 + mt * 16 + r;
    const int oy = p / a.Wo, ox = p - oy * a.Wo;
    iy0[mt] = p < P ? oy * a.stride - 1 : -4;  // a position past the map reads no tap
    ix0[mt] = ox * a.stride - 1;
  }
  f32x4 acc[4][4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[mt][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bf16x8 zero = {};
#pragma unroll
  for (int w = 0; w < T::NW; ++w) {
#pragma unroll
    for (int s = 0; s < T::NS; ++s) {
      const int j = s * 4 + h, tap = j / T::CT, cc = j % T::CT;
      const int ky = tap / 3, kx = tap - ky * 3;
      bf16x8 xb[4];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const int iy = iy0[mt] + ky, ix = ix0[mt] + kx;
        const bool ok = tap < 9 && (unsigned)iy < (unsigned)a.Hin && (unsigned)ix < (unsigned)a.Win;
        xb[mt] = ok ? *reinterpret_cast<const bf16x8*>(x + (iy * a.Win + ix) * a.C + w * KW + cc * 8) : zero;
      }
#pragma unroll
      for (int nt = 0; nt < T::NTW; ++nt) {
        const bf16x8 wf = wt[((w * T::NS + s) * T::NTW + nt) * 64];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
          acc[mt][w * T::NTW + nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xb[mt], acc[mt][w * T::NTW + nt], 0, 0, 0);
      }
    }
  }
  // D[row = output channel n * 16 + 4 h + i][col = position r]
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int c0 = n * 16 + h * 4;
    const f32x4 sc = *reinterpret_cast<const f32x4*>(a.scale + slab * 64 + c0);
    const f32x4 sh = *reinterpret_cast<const f32x4*>(a.shift + slab * 64 + c0);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int p = p0 + mt * 16 + r;
      if (p >= P) continue;
      bf16x4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float v = fmaf(acc[mt][n][i], sc[i], sh[i]);
        if (a.relu) v = fmaxf(v, 0.f);
        o[i] = (bf16_t)v;
      }
      *reinterpret_cast<bf16x4*>(y + (size_t)p * a.C + c0) = o;
    }
  }
}

__global__ __launch_bounds__(256) void conv_group_f32_kernel(GroupConvArgs a) {
  const int nq = a.C / 4, P = a.Ho * a.Wo;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= P * nq) return;
  const int p = idx / nq, n0 = (idx - p * nq) * 4, cpg = a.cpg, g0 = n0 / cpg * cpg;
  const int oy = p / a.Wo, ox = p - oy * a.Wo;
  const float* x = reinterpret_cast<const float*>(a.x) + (size_t)blockIdx.z * a.Hin * a.Win * a.C + g0;
  const float* wt = reinterpret_cast<const float*>(a.wt) + (size_t)n0 * 9 * cpg;  // [C][9][cpg]
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int tap = 0; tap < 9; ++tap) {
    const int iy = oy * a.stride - 1 + tap / 3, ix = ox * a.stride - 1 + tap % 3;
    if ((unsigned)iy >= (unsigned)a.Hin || (unsigned)ix >= (unsigned)a.Win) continue;
    const float* xr = x + (iy * a.Win + ix) * a.C;
    for (int c = 0; c < cpg; ++c) {
      const float xv = xr[c];
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = fmaf(xv, wt[(i * 9 + tap) * cpg + c], acc[i]);
    }
  }
  f32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float v = fmaf(acc[i], a.scale[n0 + i], a.shift[n0 + i]);
    o[i] = a.relu ? fmaxf(v, 0.f) : v;
  }
  *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(a.y) + ((size_t)blockIdx.z * P + p) * a.C + n0) = o;
}

bool cpg_ok(int cpg) { return cpg >= 4 && cpg <= 64 && (cpg & (cpg - 1)) == 0; }

}  // namespace

size_t conv_group_packed_bytes(DType dt, int C, int cpg) {
  if (dt != DT_BF16) return (size_t)C * 9 * cpg * sizeof(float);
  const int KW = cpg < 16 ? 16 : cpg, NS = (9 * (KW / 8) + 3) / 4;
  return (size_t)(C / 64) * (64 / KW) * NS * (KW / 16) * 64 * 8 * sizeof(uint16_t);
}

// w: detectron2's (C, cpg, 3, 3) fp32.  bf16: the MFMA A operand of every (slab, window, K step, N tile) in lane order, element j of
// lane l = W[n = window base + 16 nt + (l & 15)][k = 8 (4 s + (l >> 4)) + j] with k = tap * KW + input channel in the window, zero
// outside n's group and past the ninth tap.  fp32: [C][9][cpg].
void conv_group_pack(DType dt, const float* w, int C, int cpg, void* out) {
  if (dt != DT_BF16) {
    float* o = reinterpret_cast<float*>(out);
    for (int n = 0; n < C; ++n)
      for (int tap = 0; tap < 9; ++tap)
        for (int c = 0; c < cpg; ++c) o[((size_t)n * 9 + tap) * cpg + c] = w[((size_t)n * cpg + c) * 9 + tap];
    return;
  }
  const int KW = cpg < 16 ? 16 : cpg, CT = KW / 8, NS = (9 * CT + 3) / 4, NW = 64 / KW, NTW = KW / 16;
  bf16_t* o = reinterpret_cast<bf16_t*>(out);
  size_t i = 0;
  for (int sl = 0; sl < C / 64; ++sl)
    for (int wi = 0; wi < NW; ++wi)
      for (int s = 0; s < NS; ++s)
        for (int nt = 0; nt < NTW; ++nt)
          for (int l = 0; l < 64; ++l)
            for (int j = 0; j < 8; ++j, ++i) {
              const int base = sl * 64 + wi * KW, n = base + nt * 16 + (l & 15);
              const int chunk = s * 4 + (l >> 4), tap = chunk / CT, ci = base + (chunk % CT) * 8 + j;
              float v = 0.f;
              if (tap < 9 && ci / cpg == n / cpg) v = w[((size_t)n * cpg + ci % cpg) * 9 + tap];
              o[i] = (bf16_t)v;
            }
}

int launch_conv_group(DType dt, const GroupConvArgs& a, hipStream_t s) {
  if (a.C % 64 != 0 || !cpg_ok(a.cpg) || (a.stride != 1 && a.stride != 2) || a.B < 1 || a.B > 65535) return -1;
  if ((long)a.Hin * a.Win * a.C >= (1L << 31) || (long)a.Ho * a.Wo * a.C >= (1L << 31)) return -2;  // 32-bit offsets inside an image
  if (a.Ho != (a.Hin - 1) / a.stride + 1 || a.Wo != (a.Win - 1) / a.stride + 1) return -3;
  const int P = a.Ho * a.Wo;
  if (dt == DT_BF16) {
    const dim3 grid((P + 63) / 64, (a.C / 64 + 3) / 4, a.B);
    switch (a.cpg < 16 ? 16 : a.cpg) {
      case 16: hipLaunchKernelGGL(conv_group_bf16_kernel<16>, grid, dim3(256), 0, s, a); break;
      case 32: hipLaunchKernelGGL(conv_group_bf16_kernel<32>, grid, dim3(256), 0, s, a); break;
      default: hipLaunchKernelGGL(conv_group_bf16_kernel<64>, grid, dim3(256), 0, s, a); break;
    }
  } else {
    const long threads = (long)P * (a.C / 4);
    hipLaunchKernelGGL(conv_group_f32_kernel, dim3((unsigned)((threads + 255) / 256), 1, a.B), dim3(256), 0, s, a);
  }
  return hipGetLastError() == hipSuccess ? 0 : -4;
}

}  // namespace sylph
