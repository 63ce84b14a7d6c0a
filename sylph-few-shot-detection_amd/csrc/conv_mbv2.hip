// One whole MobileNetV2 InvertedResidual block per launch, bf16, gfx950: the 6x-expanded hidden tensor lives in LDS only.
//   y = bn(project 1x1 (relu6(bn(dw 3x3 stride s (relu6(bn(expand 1x1 (x)))))))) [+ x]            (t == 1: no expand, hidden = x)
// A workgroup of 4 waves owns an 8 x 8 tile of output positions of ONE image (grid.y = image, so a result cannot depend on where an
// image sits in the batch).  It stages the input tile with its halo ((7 s + 3)^2 positions, rows of cin_p + 8 elements) in LDS, then
// walks the hidden channels in chunks of 32:
//   a  the chunk's expand weights [32][cin_p] and projection weights [cout_p][32] -> LDS
//   b  expand on 16x16x32 MFMAs at every halo position, FrozenBN + ReLU6, ZERO where the position is outside the image (the depthwise
//      conv pads the hidden tensor, and the expand of a zero input is relu6(shift)), bf16 -> LDS
//   c  depthwise 3x3 on the VALU in fp32, the tap order of dwconv3x3_kernel, FrozenBN + ReLU6, bf16 -> LDS
//   d  projection MFMA into the accumulators: wave w owns positions 16 w .. 16 w + 15, all cout_p channels (cout_p / 16 f32x4)
// Epilogue: FrozenBN, + the input at the tile's centre positions where the block has a residual, bf16 into an LDS image of the tile
// (over the input tile), whole 16-byte lines to memory.  The rounding points are those of the three-launch chain (after the expand,
// after the depthwise conv, at the output), so the two differ by summation order only.
// MFMA operands as in conv_hpipe.hip: A = weights (row l15 = channel, 16-byte k chunk lq), B = activations (row l15 = position), so a
// lane's accumulator holds channels 4 lq .. 4 lq + 3 of position l15.
// Every global index is size_t; out-of-image positions are neither read nor stored.
#include "common.h"
#include "gfx950.h"
#include "kernels.h"

namespace sylph {

namespace {
constexpr int MB_TO = 8;        // output tile edge
constexpr int MB_HC = 32;       // hidden channels per chunk
constexpr int MB_HP = MB_HC + 8;  // LDS row pitch of the hidden chunk images and the projection weights (elements)
constexpr int MB_LDS_MAX = 160 * 1024;

struct Mbv2Lds {
  int xp, sp, np, npp;                     // input / output image row pitch (elements), halo positions, rounded up to 16
  int off_h1, off_h2, off_w1, off_w2, bytes;
};
__host__ __device__ inline Mbv2Lds mbv2_lds(int stride, int cin_p, int cout_p, int expand) {
  Mbv2Lds L;
  const int iw = (MB_TO - 1) * stride + 3;
  L.xp = cin_p + 8; L.sp = cout_p + 8;
  L.np = iw * iw; L.npp = (L.np + 15) & ~15;
  const int xin = L.npp * L.xp * 2, stage = MB_TO * MB_TO * L.sp * 2;
  L.off_h1 = xin > stage ? xin : stage;
  L.off_h2 = L.off_h1 + (expand ? L.npp * MB_HP * 2 : 0);
  L.off_w1 = L.off_h2 + MB_TO * MB_TO * MB_HP * 2;
  L.off_w2 = L.off_w1 + (expand ? MB_HC * L.xp * 2 : 0);
  L.bytes = L.off_w2 + cout_p * MB_HP * 2;
  return L;
}
__device__ __forceinline__ float mb_relu6(float v) { return fminf(fmaxf(v, 0.f), 6.f); }
}  // namespace

template <int NT>
__global__ void __launch_bounds__(256) conv_mbv2_kernel(Mbv2Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mb_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lq = lane >> 4;
  const int expand = a.w1 != nullptr;
  const Mbv2Lds L = mbv2_lds(a.stride, a.cin_p, NT * 16, expand);
  bf16_t* xin = (bf16_t*)mb_smem;
  bf16_t* h1 = (bf16_t*)(mb_smem + L.off_h1);
  bf16_t* h2 = (bf16_t*)(mb_smem + L.off_h2);
  bf16_t* w1s = (bf16_t*)(mb_smem + L.off_w1);
  bf16_t* w2s = (bf16_t*)(mb_smem + L.off_w2);
  const int tiles_x = (a.Wo + MB_TO - 1) / MB_TO;
  const int oy0 = (int)(blockIdx.x / tiles_x) * MB_TO, ox0 = (int)(blockIdx.x % tiles_x) * MB_TO, b = blockIdx.y;
  const int iy0 = oy0 * a.stride - 1, ix0 = ox0 * a.stride - 1, IW = (MB_TO - 1) * a.stride + 3;
  const bf16_t* xb = (const bf16_t*)a.x + (size_t)b * a.H * a.W * a.cin_ld;

  // the input tile with its halo; zeros outside the image and in the rows that round the position count up to 16
  {
    const int cpr = a.cin_p >> 3;
    for (int i = tid; i < L.npp * cpr; i += 256) {
      const int p = i / cpr, ck = i - p * cpr, iy = iy0 + p / IW, ix = ix0 + p % IW;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (p < L.np && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) v = *(const uint4*)(xb + ((size_t)iy * a.W + ix) * a.cin_ld + ck * 8);
      *(uint4*)(xin + p * L.xp + ck * 8) = v;
    }
  }
  f32x4 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nchunks = a.hid_p / MB_HC, ksteps = a.cin_p >> 5;
  for (int c = 0; c < nchunks; ++c) {
    const int hc0 = c * MB_HC;
    // a: this chunk's weights
    if (expand) {
      const int cpr = a.cin_p >> 3;
      for (int i = tid; i < MB_HC * cpr; i += 256) {
        const int r = i / cpr, ck = i - r * cpr;
        *(uint4*)(w1s + r * L.xp + ck * 8) = *(const uint4*)(a.w1 + (size_t)(hc0 + r) * a.cin_p + ck * 8);
      }
    }
    for (int i = tid; i < NT * 16 * 4; i += 256) {
      const int n = i >> 2, ck = i & 3;
      *(uint4*)(w2s + n * MB_HP + ck * 8) = *(const uint4*)(a.w2 + (size_t)n * a.hid_p + hc0 + ck * 8);
    }
    __syncthreads();
    // b: expand at every halo position
    if (expand) {
      for (int mt = wave; mt < (L.npp >> 4); mt += 4) {
        f32x4 e0 = f32x4{0.f, 0.f, 0.f, 0.f}, e1 = e0;
        const bf16_t* xr = xin + (mt * 16 + l15) * L.xp + lq * 8;
        const bf16_t* wr = w1s + l15 * L.xp + lq * 8;
        for (int ks = 0; ks < ksteps; ++ks) {
          const bf16x8 fa = *(const bf16x8*)(xr + ks * 32);
          const bf16x8 f0 = *(const bf16x8*)(wr + ks * 32), f1 = *(const bf16x8*)(wr + 16 * L.xp + ks * 32);
          e0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f0, fa, e0, 0, 0, 0);
          e1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f1, fa, e1, 0, 0, 0);
        }
        const int p = mt * 16 + l15, iy = iy0 + p / IW, ix = ix0 + p % IW;
        const bool inside = p < L.np && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const f32x4 e = j ? e1 : e0;
          const int ch = hc0 + j * 16 + lq * 4;
          const float4 sc = *(const float4*)(a.s1 + ch), sh = *(const float4*)(a.b1 + ch);
          alignas(8) bf16_t o[4];
          o[0] = (bf16_t)(inside ? mb_relu6(fmaf(e[0], sc.x, sh.x)) : 0.f);
          o[1] = (bf16_t)(inside ? mb_relu6(fmaf(e[1], sc.y, sh.y)) : 0.f);
          o[2] = (bf16_t)(inside ? mb_relu6(fmaf(e[2], sc.z, sh.z)) : 0.f);
          o[3] = (bf16_t)(inside ? mb_relu6(fmaf(e[3], sc.w, sh.w)) : 0.f);
          *(uint2*)(h1 + p * MB_HP + j * 16 + lq * 4) = *(const uint2*)o;
        }
      }
      __syncthreads();
    }
    // c: depthwise 3x3: a thread owns 8 channels of one output position
    {
      const int o = tid >> 2, cg = (tid & 3) * 8, oy = o >> 3, ox = o & 7;
      const bf16_t* src = expand ? h1 + cg : xin + hc0 + cg;
      const int pitch = expand ? MB_HP : L.xp;
      float d[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) d[i] = 0.f;
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          float v[8], w[8];
          load8<bf16_t>(src + ((oy * a.stride + kh) * IW + ox * a.stride + kw) * pitch, v);
          load8<float>(a.wd + (size_t)(kh * 3 + kw) * a.hid_p + hc0 + cg, w);
#pragma unroll
          for (int i = 0; i < 8; ++i) d[i] = fmaf(mb_relu6(v[i]), w[i], d[i]);
        }
      float sc[8], sh[8], r[8];
      load8<float>(a.sd + hc0 + cg, sc);
      load8<float>(a.bd + hc0 + cg, sh);
#pragma unroll
      for (int i = 0; i < 8; ++i) r[i] = mb_relu6(fmaf(d[i], sc[i], sh[i]));
      store8<bf16_t>(h2 + o * MB_HP + cg, r);
    }
    __syncthreads();
    // d: projection, K = this chunk
    {
      const bf16x8 fa = *(const bf16x8*)(h2 + (wave * 16 + l15) * MB_HP + lq * 8);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const bf16x8 fb = *(const bf16x8*)(w2s + (nt * 16 + l15) * MB_HP + lq * 8);
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb, fa, acc[nt], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // epilogue: FrozenBN [+ x], through an LDS image of the output tile (over the input tile: every read of it is done after the barrier)
  const int o = wave * 16 + l15, oy = o >> 3, ox = o & 7;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int ch = nt * 16 + lq * 4;
    const float4 sc = *(const float4*)(a.s2 + ch), sh = *(const float4*)(a.b2 + ch);
    acc[nt][0] = fmaf(acc[nt][0], sc.x, sh.x);
    acc[nt][1] = fmaf(acc[nt][1], sc.y, sh.y);
    acc[nt][2] = fmaf(acc[nt][2], sc.z, sh.z);
    acc[nt][3] = fmaf(acc[nt][3], sc.w, sh.w);
    if (a.residual) {  // (stride 1, cin_p == cout_p: the tile's centre positions)
      const bf16_t* r = xin + ((oy + 1) * IW + ox + 1) * L.xp + ch;
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[nt][e] += (float)r[e];
    }
  }
  __syncthreads();
  bf16_t* stage = (bf16_t*)mb_smem;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    alignas(8) bf16_t v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (bf16_t)acc[nt][e];
    *(uint2*)(stage + o * L.sp + nt * 16 + lq * 4) = *(const uint2*)v;
  }
  __syncthreads();
  {
    bf16_t* yb = (bf16_t*)a.y + (size_t)b * a.Ho * a.Wo * a.cout_ld;
    const int cpr = NT * 2;
    for (int i = tid; i < MB_TO * MB_TO * cpr; i += 256) {
      const int q = i / cpr, ck = i - q * cpr, yy = oy0 + (q >> 3), xx = ox0 + (q & 7);
      if (yy < a.Ho && xx < a.Wo) *(uint4*)(yb + ((size_t)yy * a.Wo + xx) * a.cout_ld + ck * 8) = *(const uint4*)(stage + q * L.sp + ck * 8);
    }
  }
}

// what the kernel can run: bf16 operands packed by make_mbv2_block, the channel counts of the MobileNetV2 table as stored
bool conv_mbv2_can_run(const Mbv2Args& a) {
  if (!a.x || !a.y || !a.w2 || !a.s2 || !a.b2 || !a.wd || !a.sd || !a.bd || (a.w1 && (!a.s1 || !a.b1))) return false;
  if (a.B < 1 || a.B > 65535 || a.H < 1 || a.W < 1 || (a.stride != 1 && a.stride != 2)) return false;
  if (a.Ho != (a.H - 1) / a.stride + 1 || a.Wo != (a.W - 1) / a.stride + 1) return false;
  if (a.cin_p < 32 || (a.cin_p & 31) || a.hid_p < MB_HC || (a.hid_p % MB_HC) || a.cin_ld < a.cin_p || (a.cin_ld & 7) || a.cout_ld < a.cout_p || (a.cout_ld & 7)) return false;
  if (!a.w1 && a.hid_p != a.cin_p) return false;
  if (a.cout_p != 64 && a.cout_p != 128 && a.cout_p != 192 && a.cout_p != 320) return false;
  if (a.residual && (a.stride != 1 || a.cin_p != a.cout_p)) return false;
  return mbv2_lds(a.stride, a.cin_p, a.cout_p, a.w1 != nullptr).bytes <= MB_LDS_MAX;
}

template <int NT>
static int launch_mbv2_nt(const Mbv2Args& a, int lds, dim3 grid, hipStream_t s) {
  static PerDeviceOnce once;
  if (!once.run(current_device(), [] { return hipFuncSetAttribute((const void*)conv_mbv2_kernel<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, MB_LDS_MAX) == hipSuccess; }))
    return -7;
  hipLaunchKernelGGL(conv_mbv2_kernel<NT>, grid, dim3(256), lds, s, a);
  return (int)hipGetLastError();
}

int launch_conv_mbv2(const Mbv2Args& a, hipStream_t s) {
  if (!conv_mbv2_can_run(a)) return -4;
  const size_t tiles = (size_t)((a.Ho + MB_TO - 1) / MB_TO) * ((a.Wo + MB_TO - 1) / MB_TO);
  if (tiles > 0x7fffffffu) return -5;
  const int lds = mbv2_lds(a.stride, a.cin_p, a.cout_p, a.w1 != nullptr).bytes;
  const dim3 grid((unsigned)tiles, (unsigned)a.B);
  switch (a.cout_p) {
    case 64: return launch_mbv2_nt<4>(a, lds, grid, s);
    case 128: return launch_mbv2_nt<8>(a, lds, grid, s);
    case 192: return launch_mbv2_nt<12>(a, lds, grid, s);
    default: return launch_mbv2_nt<20>(a, lds, grid, s);
  }
}

}  // namespace sylph
