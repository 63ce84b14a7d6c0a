// gfx950 (CDNA4) device primitives shared by the hand-scheduled kernels: address-space pointer and ext-vector typedefs, barriers,
// counted waits, and the inline-asm MFMAs with the weight operand in an AGPR.  Device code only.
#pragma once
#include "common.h"

namespace sylph {

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* gbl_ptr_t;

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));  // ext_vector LDS accesses: hipcc adds no vmcnt(0) for them beside LDS-DMA
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef float f32x2 __attribute__((ext_vector_type(2)));

// ---- barriers ------------------------------------------------------------------------------------------------------------
// keeps the scheduler from moving any instruction across this point
__device__ __forceinline__ void sched_fence() { __builtin_amdgcn_sched_barrier(0); }

// Raw s_barrier that neither the compiler's memory model nor the scheduler moves anything across, and that waits for nothing:
// the pipelined kernels retire their loads with counted waits of their own.
__device__ __forceinline__ void fenced_barrier() {
  asm volatile("" ::: "memory");
  sched_fence();
  __builtin_amdgcn_s_barrier();
  sched_fence();
  asm volatile("" ::: "memory");
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains vmcnt, i.e. waits for every global
// store (and prefetch load) still in flight: ~1-2 us per barrier in an epilogue that has just issued its stores.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// ---- counted waits -------------------------------------------------------------------------------------------------------
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
__device__ __forceinline__ void wait_lgkmcnt0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// s_waitcnt vmcnt(min(n, MAX)) for a wave-uniform run-time n >= 0 (the instruction takes an immediate); the cases from MAX on
// fall through to the default
template <int MAX> __device__ __forceinline__ void wait_vmcnt_upto(int n) {
  static_assert(MAX >= 1 && MAX <= 63, "vmcnt range");
  switch (n) {
#define GFX950_WAIT_CASE(N) \
  case N:                   \
    if constexpr (N < MAX) { wait_vmcnt<N>(); break; }
    GFX950_WAIT_CASE(0) GFX950_WAIT_CASE(1) GFX950_WAIT_CASE(2) GFX950_WAIT_CASE(3) GFX950_WAIT_CASE(4) GFX950_WAIT_CASE(5)
    GFX950_WAIT_CASE(6) GFX950_WAIT_CASE(7) GFX950_WAIT_CASE(8) GFX950_WAIT_CASE(9) GFX950_WAIT_CASE(10) GFX950_WAIT_CASE(11)
    GFX950_WAIT_CASE(12) GFX950_WAIT_CASE(13) GFX950_WAIT_CASE(14) GFX950_WAIT_CASE(15) GFX950_WAIT_CASE(16) GFX950_WAIT_CASE(17)
    GFX950_WAIT_CASE(18) GFX950_WAIT_CASE(19) GFX950_WAIT_CASE(20) GFX950_WAIT_CASE(21) GFX950_WAIT_CASE(22) GFX950_WAIT_CASE(23)
    GFX950_WAIT_CASE(24) GFX950_WAIT_CASE(25) GFX950_WAIT_CASE(26) GFX950_WAIT_CASE(27) GFX950_WAIT_CASE(28) GFX950_WAIT_CASE(29)
    GFX950_WAIT_CASE(30) GFX950_WAIT_CASE(31) GFX950_WAIT_CASE(32) GFX950_WAIT_CASE(33) GFX950_WAIT_CASE(34) GFX950_WAIT_CASE(35)
    GFX950_WAIT_CASE(36) GFX950_WAIT_CASE(37) GFX950_WAIT_CASE(38) GFX950_WAIT_CASE(39) GFX950_WAIT_CASE(40) GFX950_WAIT_CASE(41)
    GFX950_WAIT_CASE(42) GFX950_WAIT_CASE(43) GFX950_WAIT_CASE(44) GFX950_WAIT_CASE(45) GFX950_WAIT_CASE(46) GFX950_WAIT_CASE(47)
    GFX950_WAIT_CASE(48) GFX950_WAIT_CASE(49) GFX950_WAIT_CASE(50) GFX950_WAIT_CASE(51) GFX950_WAIT_CASE(52) GFX950_WAIT_CASE(53)
    GFX950_WAIT_CASE(54) GFX950_WAIT_CASE(55) GFX950_WAIT_CASE(56) GFX950_WAIT_CASE(57) GFX950_WAIT_CASE(58) GFX950_WAIT_CASE(59)
    GFX950_WAIT_CASE(60) GFX950_WAIT_CASE(61) GFX950_WAIT_CASE(62)
#undef GFX950_WAIT_CASE
    default: wait_vmcnt<MAX>(); break;
  }
}

// ---- MFMA with the weight fragment in an AGPR --------------------------------------------------------------------------
// MFMA with the weight fragment read straight from an AGPR and the accumulator in arch VGPRs.  Through the builtin hipcc keeps
// weights and accumulators in AGPRs only as spill space and pays a v_accvgpr_read per use (~450 per tile, all on the one wave
// that also has to issue the MFMAs).  Inline asm is invisible to the hazard recogniser: mfma_drain before the first VALU
// read of an accumulator supplies the wait states (16-pass MFMA: 18) it would have inserted.
__device__ __forceinline__ void mfma_aw(f32x16& acc, const bf16x8& w, const bf16x8& av) {
  asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "a"(w), "v"(av));
}
// first k-step of a chain: srcC = 0 (a VALU zero-fill followed by an MFMA reading it is a 2-wait-state hazard nobody would pad)
__device__ __forceinline__ void mfma_aw0(f32x16& acc, const bf16x8& w, const bf16x8& av) {
  asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, 0" : "=&v"(acc) : "a"(w), "v"(av));
}
// the same with the weight fragment in VGPRs
__device__ __forceinline__ void mfma_vw(f32x16& acc, const bf16x8& w, const bf16x8& av) {
  asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(w), "v"(av));
}
// (the accumulators are operands of the drain: their VALU reads must not be scheduled above it.  Asm operands cannot come from a
// parameter pack: one overload per arity)
__device__ __forceinline__ void mfma_drain(f32x16& a0, f32x16& a1) { asm volatile("s_nop 15\n\ts_nop 3" : "+v"(a0), "+v"(a1)::"memory"); }
__device__ __forceinline__ void mfma_drain(f32x16& a0, f32x16& a1, f32x16& a2) {
  asm volatile("s_nop 15\n\ts_nop 3" : "+v"(a0), "+v"(a1), "+v"(a2)::"memory");
}
__device__ __forceinline__ void mfma_drain(f32x16& a0, f32x16& a1, f32x16& a2, f32x16& a3) {
  asm volatile("s_nop 15\n\ts_nop 3" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3)::"memory");
}

}  // namespace sylph
