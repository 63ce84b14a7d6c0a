// Deep-pipelined 3x3 (stride 1, pad 1) implicit-GEMM convolution with a HALO A operand, for the MFMA-bound layers
// (FCOS towers fcos.py:72-122, FPN output convs, bottleneck conv2 of res4/res5).
//
// One 512-thread block per CU owns a 256 (positions) x 256 (channels) output tile.  The 256 positions are TWO
// independent ph x pw patches (<= 128 positions each, shapes picked per pyramid level on the host: 10 x 12 on the
// 100 x 168 / 50 x 84 maps), one per wave row:
//
//   * 8 waves = 2 (patch) x 4 (64-channel column); wave tile 128 x 64 = 8 x 4 MFMA 16x16x32 tiles (128 accumulator
//     VGPRs): one k-step of 32 per tap, 12 ds_read_b128 (8 position + 4 weight fragments, 48 VGPRs) per 32 MFMAs.  This
//     kernel's instruction mix on random data sustains 1.175x the FLOP/s in the 16x16x32 form (profiles/r7_mfma_shape_probe.txt);
//     in the kernel the change measured as 6-11 % fewer cycles at an unchanged clock (profiles/r7_clock_counters.txt).
//   * K order: 32-channel half-slice outer, the 9 taps inner.  A operand: the (ph+2) x (pw+2) input halo of each patch
//     for one half-slice (64-byte rows) is fetched ONCE and all nine taps read shifted rows of it, so the only per-tap
//     traffic is the weight tile (256 rows x 64 B = 16 KiB): L2->LDS bytes per flop are 0.58x those of a plain
//     256x256 GEMM tile (the round-1 conv_pipe kernel starved on exactly that stream) and 0.36x those of the
//     128x128 halo kernel.
//   * LDS: four 16-KiB weight stages (ring) + two 32-KiB halo buffers (double buffer) = 128 KiB.  The weight tile of
//     phase q+3 and (during taps 0..3) one quarter of the next half-slice's halo are issued by global_load_lds right after
//     the fragment reads of phase q and waited for two phases later with a COUNTED s_waitcnt vmcnt(N): never a drain in
//     the steady state.  The 9 taps are unrolled, so every N and every tap offset is an immediate.  The loads sit in the
//     L (fragment read) segment, whose instruction stream has the slack; the M segment is 32 bare MFMAs.  Load addresses
//     cost no VALU work: weights use a wave-uniform base + a constant per-lane offset, the halo running per-lane pointers.
//   * The two wave rows (the two waves that share a SIMD) run staggered by one barrier: while one issues its 32
//     MFMAs (s_setprio 1) the other does its fragment reads and address arithmetic.  Raw s_barrier + explicit
//     waitcnts only (a __syncthreads would drain the LDS-DMA queue).
//
// Hazards (B_n = n-th barrier, seg n = between B_n and B_n+1; row 0 does L(q) in seg 2q and M(q) in seg 2q+1, row 1 one
// segment later):
//   RAW  weight stage of phase q+1 (issued in L(q-2)) is read from seg 2q+2 on; both rows execute their vmcnt wait for
//        their own phase-(q+1) loads in seg 2q+1 (row 0 at the end of M(q), row 1 at the end of L(q)), i.e. before B_{2q+2}.
//        The halo of half-slice c+1 is issued in L(c,0..3); the in-order vmcnt waits of phases (c,4..6) retire it long
//        before L(c+1,0).
//   WAR  stage (q-1)&3 (and, at tap 0, the halo buffer last read in L(q-1)) is refilled by row 0 in seg 2q and by row 1 in
//        seg 2q+1; the last reader (row 1, L(q-1), seg 2q-1) retires its ds_reads with lgkmcnt(0) before B_{2q}.
//
// Weights are RE-PACKED for this kernel (hpipe_pack_weights_kernel, once per layer): [n tile][half-slice][tap] -> one
// contiguous 16-KiB block that already is the LDS image of a stage.  With the generic [n][kh][kw][c] layout the 256 rows of
// a phase sit 4 608 B apart: every phase touched the same 4 of the 16 L2 channels, in half cache lines, from all CUs at
// once, and the kernel ran 32 % slower than with the loads removed.  Now a stage is a linear 16-KiB copy (128 full lines
// over all channels).  Blocks also start the K loop at different half-slices (rotation by tile index), which spreads the
// 64-byte-per-512-byte halo rows of concurrently running blocks over the channels.
//
// LDS images (lane-linear global_load_lds, swizzle on the SOURCE side, same XOR on the fragment reads).  A 16x16x32 operand
// read gives lane l row l & 15 and 16-byte chunk c = l >> 4; the 16 lanes of a ds_read_b128 group are rows {0-3, 12-15}
// with chunk c0 and rows {4-11} with chunk c0 ^ 1 ({0-3, 12-15, 20-27}: c0 = 0, {4-11, 16-19, 28-31}: c0 = 1, + 32: c0 ^ 2).
// With 64-byte rows the 16-byte bank slot of slot s in a row with key x is (x & 3) * 4 + s (below: the row index equals the
// key mod 4), so the four lanes of one key residue, keys x, x + 12 (chunk c0) and x + 4, x + 8 (chunk c0 ^ 1) for some x,
// need four distinct slots.  The swizzle
//   slot = chunk ^ sw(key),  sw(key) = ((key >> 2) & 1) << 1
// gives them c0 ^ {a, a ^ 2} and c0 ^ 1 ^ {a ^ 2, a}: distinct, for EVERY x, so a read stays conflict-free when all its
// keys are shifted by the same amount.  (The 32x32x16 swizzle chunk ^ ((key >> 2) & 3) is 2-way on this read pattern.)
//   weights [256 rows][64 B]: key = row r (applied by the re-pack);
//   halo    [2 patches][256 rows][64 B], row h = hy * (pw + 4) + hx: key k = hy * pw + hx.  The reader of tap (kh, kw) at patch
//           position m sits on k = m + kh * pw + kw, and with the pitch pw + 4 (two unused entries per halo row) h = k + 4 hy,
//           so h & 3 = k & 3 and a read's slots depend on (m + kh * pw + kw) mod 16 only: conflict-free for every tap and
//           every patch shape (tests/test_hpipe_mfma16_swizzle.py enumerates them).  (Pitch pw + 2 made the slot depend on
//           the parity of hy: measured 35 % of all LDS cycles were bank conflicts, SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE.)
//
// Scope (launch_conv checks): bf16 in/out, 3x3 s1 p1, no residual, no per-segment Scale, ReLU on all channels or none,
// Cout % 256 == 0, Cin % 32 == 0, padded scale/shift; optional fused GroupNorm partial statistics (one per patch).
#include "gfx950.h"

namespace sylph {

namespace {
constexpr int PNT = 512;
constexpr int BSTAGE = 256 * 64;               // one weight stage: 256 output channels x 32 input channels
constexpr int NSTAGE = 4;
constexpr int HPROWS = 256;                    // halo rows reserved per patch
constexpr int HBUF = 2 * HPROWS * 64;          // one halo buffer (both patches)
constexpr int HALO_OFF = NSTAGE * BSTAGE;
constexpr int COEF_OFF = HALO_OFF + 2 * HBUF;   // fused input GroupNorm: (a, b) per patch and input channel, [2][Cin] float2
constexpr int COEF_MAX_CIN = 512;
constexpr int LDS_BYTES = COEF_OFF + 2 * COEF_MAX_CIN * 8;  // 139 264
constexpr int SCP = 256 + 4;                   // fp32 pitch of the epilogue tile
static_assert(64 * SCP * 4 <= LDS_BYTES, "epilogue tile must fit");

// loads a wave issues in the L segment of tap t: the two weight halves of phase q+3, plus one halo piece on taps 0..3
constexpr int NPIECE = 2 * HPROWS / 128;  // block-wide halo loads per half-slice (taps 0..3 carry one each)
constexpr int nload(int t) { return ((t % 9 + 9) % 9) < NPIECE ? 3 : 2; }

}  // namespace

template <bool GNIN>
__global__ __launch_bounds__(PNT, 1) void conv_hpipe_kernel(const ConvArgs a) {
  typedef bf16_t T;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  // XCD-aware block -> tile map (as conv_igemm.hip); an M tile is a PAIR of patches
  const int L = blockIdx.x;
  const int xcd = L & 7, q0 = L >> 3;
  const int chunk = (a.n_mtiles + 7) >> 3;
  const int m_local = q0 / a.n_ntiles;
  const int nt = q0 - m_local * a.n_ntiles;
  const int mt = xcd * chunk + m_local;
  if (m_local >= chunk || mt >= a.n_mtiles) return;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int l15 = lane & 15, lq = lane >> 4;  // MFMA 16x16x32 operand row / 16-byte k chunk of this lane

  int2 tl0 = a.tiles[2 * mt], tl1 = a.tiles[2 * mt + 1];
  const int rot_key = (int)((unsigned)tl0.x >> 20);  // index of this pair inside its image (api_conv.hip make_geom_patch)
  tl0.x &= 0xfffff;
  const SegDesc sd0 = a.segs[tl0.x], sd1 = a.segs[tl1.x];

  const T* __restrict__ in = reinterpret_cast<const T*>(a.in);
  const T* __restrict__ wt = reinterpret_cast<const T*>(a.wt);
  const T* __restrict__ zero = reinterpret_cast<const T*>(a.zeros);
  const int Cin = a.Cin;
  const int ncc = Cin >> 5;  // 32-channel half-slices
  // K-loop rotation: this block walks the half-slices c0, c0+1, ... (mod ncc); keyed on the pair's place inside its own image, so the
  // summation order of an image's outputs does not depend on the batch around it
  const int c0 = (rot_key + nt) % ncc;

  // ---- loader state --------------------------------------------------------------------------------------------
  // lane (r4, s4) of a block-wide global_load_lds fetches 16-byte slot s4 of LDS row (round * 128 + r4)
  const int r4 = tid >> 2, s4 = tid & 3;
  // halo: LDS rows [0, 256) patch 0, [256, 512) patch 1; four rounds of 128 rows, halo row (hy, hx) at hy * hpitch + hx.
  // Each lane keeps a running 64-bit source pointer per halo piece (advanced by 64 B per half-slice; lanes outside the
  // image / past the halo stay on the zero page), so issuing a piece costs no VALU work.
  const char* hptr[NPIECE];
  unsigned hmask = 0, hcs = 0;  // per piece: inside the image?  / logical 16-byte chunk (8 channels) this lane fetches
#pragma unroll
  for (int g = 0; g < NPIECE; ++g) {
    const bool p1 = g >= NPIECE / 2;
    const SegDesc& sd = p1 ? sd1 : sd0;
    const int ty = p1 ? tl1.y : tl0.y;
    const int h = g * 128 + r4 - (p1 ? HPROWS : 0);
    const int PW = sd.pw, HP = sd.hpitch, HR = (sd.ph + 2) * HP;
    const int hy = (int)(((unsigned)h * sd.inv_hw2) >> 16), hx = h - hy * HP;
    const int iy = (ty >> 16) - 1 + hy, ix = (ty & 0xffff) - 1 + hx;
    const bool ok = h < HR && hx < PW + 2 && (unsigned)iy < (unsigned)sd.in_H && (unsigned)ix < (unsigned)sd.in_W;
    const int cs = s4 ^ ((((hy * PW + hx) >> 2) & 1) << 1);
    hcs |= (unsigned)cs << (2 * g);
    hptr[g] = ok ? reinterpret_cast<const char*>(in + ((size_t)(sd.in_row0 + iy * sd.in_W + ix) * a.in_ld + cs * 8 + c0 * 32))
                 : reinterpret_cast<const char*>(zero + s4 * 8);
    hmask |= (ok ? 1u : 0u) << g;
  }
  // weights: stage image of (n tile, half-slice c, tap t) = 16 KiB at ((nt * ncc + c) * 9 + t) * 16 KiB; lane copies
  // bytes [tid * 16, +16) of each 8-KiB half: wave-uniform base (SALU) + a constant per-lane offset
  const char* const wtile = reinterpret_cast<const char*>(wt) + (size_t)nt * ncc * 9 * BSTAGE;
  const unsigned wvo = (unsigned)tid * 16u;
  auto issue_halo = [&](int g, int buf) {  // piece g of the half-slice the running pointers stand on -> halo buffer buf
    char* d = smem + HALO_OFF + buf * HBUF + g * 8192 + wave * 1024;  // wave-uniform; lane l lands at +16 l
    __builtin_amdgcn_global_load_lds((gbl_ptr_t)hptr[g], (lds_ptr_t)d, 16, 0, 0);
  };
  // step the halo pointers to the next half-slice of the rotated walk (wrap: back by Cin - 32 channels)
  auto advance_halo = [&](int cc_next) {
    const int step = (c0 + cc_next == ncc) ? (32 - Cin) * 2 : 64;  // wave-uniform
#pragma unroll
    for (int g = 0; g < NPIECE; ++g) hptr[g] += ((hmask >> g) & 1u) ? step : 0;
  };
  // Always true.  The guard folds away, yet without it hipcc moves the weight loads' address arithmetic through the K loop
  // from VALU to SALU: a schedule change to be measured on its own, not part of the refactor that removed its other uses.
  bool w_loads = true;
  auto issue_w = [&](int stage, int j, int blk) {  // 8-KiB half j of weight block blk (= rotated half-slice * 9 + tap)
    if (!w_loads) return;
    char* d = smem + stage * BSTAGE + j * 8192 + wave * 1024;
    const char* src = wtile + (size_t)blk * BSTAGE + j * 8192 + wvo;
    __builtin_amdgcn_global_load_lds((gbl_ptr_t)src, (lds_ptr_t)d, 16, 0, 0);
  };
  auto rot = [&](int cc) { const int c = c0 + cc; return c >= ncc ? c - ncc : c; };

  // Fused GroupNorm(+ReLU) of the input (a.gn_coef): every lane rewrites, in LDS, exactly the 16 bytes (8 channels of one
  // halo position) it fetched itself -- so the only ordering it needs is its own vmcnt wait for that load -- as
  // bf16(relu(a * x + b)).  Lanes on the zero page (conv padding, halo pad entries) are skipped: the padding of the
  // NORMALISED tensor is zero.  Readers see the result after the next lgkmcnt(0) + barrier, phases before its first use.
  constexpr bool gn_in = GNIN;  // the plain instantiation carries none of this
  // ReLU (or none) on a bf16 pair as a packed signed 16-bit max with a wave-uniform floor: 0 clears negative values (sign bit set),
  // -32768 passes every value.  Unconditional, so the transform carries no select between the two forms (fewer VALU per MFMA gap).
  const short gn_floor = a.gn_relu != 0 ? (short)0 : (short)-32768;
  // The LDS accesses are inline asm: for a compiler-visible ds_read hipcc inserts s_waitcnt vmcnt(0) (it must assume the
  // LDS-DMA still in flight aliases the read), which would drain the whole load pipeline in 4 of 9 phases.  The data read
  // here was fetched by THIS lane and retired by this wave's counted vmcnt two phases ago; the lgkmcnt wait is tied to the
  // loaded registers ("+v") so that no consumer can be scheduled above it.
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
  u32x4 gx;
  f32x4 gc0, gc1, gc2, gc3;  // (a, b) pairs of channels (0,1) (2,3) (4,5) (6,7)
  auto gn_addr = [&](int g, int cc_of_piece) { return lds0 + HALO_OFF + (cc_of_piece & 1) * HBUF + g * 8192 + tid * 16; };
  auto gn_read = [&](int g, int cc_of_piece) {  // issue the five LDS reads of piece g (no wait)
    const unsigned d = gn_addr(g, cc_of_piece);
    const int ch = rot(cc_of_piece) * 32 + (int)((hcs >> (2 * g)) & 3u) * 8;
    const unsigned cf = lds0 + COEF_OFF + ((g >= NPIECE / 2 ? Cin : 0) + ch) * 8;
    asm volatile("ds_read_b128 %0, %1" : "=v"(gx) : "v"(d));
    asm volatile("ds_read_b128 %0, %1" : "=v"(gc0) : "v"(cf));
    asm volatile("ds_read_b128 %0, %1 offset:16" : "=v"(gc1) : "v"(cf));
    asm volatile("ds_read_b128 %0, %1 offset:32" : "=v"(gc2) : "v"(cf));
    asm volatile("ds_read_b128 %0, %1 offset:48" : "=v"(gc3) : "v"(cf));
  };
  auto gn_finish = [&](int g, int cc_of_piece) {  // wait for them, transform, write back (branch-free: no cut in the MFMA stream)
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(gx), "+v"(gc0), "+v"(gc1), "+v"(gc2), "+v"(gc3));
    const unsigned live = ((hmask >> g) & 1u) ? 0xffffffffu : 0u;  // zero-page lanes (conv padding) keep their zeros
    const f32x4 cs[4] = {gc0, gc1, gc2, gc3};                      // per channel pair: (a_lo, a_hi, b_lo, b_hi)
    u32x4 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const f32x2 xv = {__uint_as_float(gx[e] << 16), __uint_as_float(gx[e] & 0xffff0000u)};
      const f32x2 av = {cs[e][0], cs[e][1]}, bv = {cs[e][2], cs[e][3]};
      const f32x2 r = __builtin_elementwise_fma(xv, av, bv);
      const bf16x2 pk = __builtin_convertvector(r, bf16x2);  // one v_cvt_pk_bf16_f32 (round to nearest even, as the casts)
      const s16x2 fl = {gn_floor, gn_floor};
      const unsigned u = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(s16x2, pk), fl));
      y[e] = u & live;
    }
    asm volatile("ds_write_b128 %0, %1" ::"v"(gn_addr(g, cc_of_piece)), "v"(y) : "memory");
  };
  auto gn_piece = [&](int g, int cc_of_piece) { gn_read(g, cc_of_piece); gn_finish(g, cc_of_piece); };

  // ---- fragment addressing -----------------------------------------------------------------------------------------
  const SegDesc& sdm = wm ? sd1 : sd0;  // this wave row's patch
  const int PWm = sdm.pw, HW2m = sdm.hpitch;
  int a0[8];  // position fragment i: patch position m = 16 i + l15
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int m = i * 16 + l15;
    const int my = (int)(((unsigned)m * sdm.inv_pw) >> 16);
    a0[i] = (wm * HPROWS + my * HW2m + (m - my * PWm)) * 64;
  }
  // weight fragment j: output channel wn * 64 + 16 j + l15 (16 j keeps the row's swizzle key)
  const int offB = (wn * 64 + l15) * 64 + ((lq ^ (((l15 >> 2) & 1) << 1)) << 4);

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;
  bf16x8 fa[8], fb[4];

  // L(cc, t): the 12 fragment reads of tap t of half-slice cc
  auto ldfrag = [&](int cc, int t) {
    const int kh = t / 3, kw = t - 3 * kh;
    const char* bs = smem + ((cc + t) & 3) * BSTAGE;  // phase q = 9 cc + t; q & 3 == (cc + t) & 3
    const char* hs = smem + HALO_OFF + (cc & 1) * HBUF + (kh * HW2m + kw) * 64;
    // swizzle key k = 16 i + l15 + kh * pw + kw: bit 2 of it does not depend on i.  Recomputed per tap (three VALU): hoisted
    // out of the K loop, the nine per-tap values cost nine VGPRs the kernel does not have (they were spilled to scratch).
    int key = l15;
    asm volatile("" : "+v"(key));
    const int so = (lq ^ ((((key + kh * PWm + kw) >> 2) & 1) << 1)) << 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) fb[j] = *reinterpret_cast<const bf16x8*>(bs + offB + j * 1024);
#pragma unroll
    for (int i = 0; i < 8; ++i) fa[i] = *reinterpret_cast<const bf16x8*>(hs + a0[i] + so);
  };

  // The loads of phase q+3 = tap t+3 (weights into stage (q+3) & 3) and, on taps 0..2, piece t of the next half-slice's
  // halo.  Issued in the L segment, after the fragment reads: the other wave row is in its MFMA segment meanwhile.
  // Past the last phase the weight loads re-read K offset 0 into a stage nobody reads any more (constant load count).
  auto issue_next = [&](int cc, int t) {
    const int t3 = (t + 3) % 9, cc3 = cc + (t + 3) / 9;
    const int blk = cc3 < ncc ? rot(cc3) * 9 + t3 : 0;
    const int st3 = (cc + t + 3) & 3;
    if (t == 0 && cc + 1 < ncc) advance_halo(cc + 1);  // the pointers now stand on (rotated) half-slice cc + 1; the last one is re-read at the end: harmless
    if (t < NPIECE) issue_halo(t, (cc + 1) & 1);
    issue_w(st3, 0, blk);
    issue_w(st3, 1, blk);
  };
  // M(cc, t): 32 back-to-back MFMAs.  With a fused input GroupNorm, taps 3..6 also transform halo piece t - 3 of the next
  // half-slice (landed: its load was issued in L(cc, t - 3) and retired by this wave's counted wait two phases later); the
  // ~30 VALU / LDS instructions are spread between the MFMAs (sched_group_barrier), where the wave has free issue slots.  A
  // 16x16x32 MFMA holds the SIMD's issue for 8 of its 16 cycles, which leaves room for about two 4-cycle VALU per gap (shared
  // with the partner wave's L segment): the transform goes at most two per gap over MFMAs 8..23.  (Its 32x32x16 form had ~40
  // VALU at four per gap; packed at three per gap here it cost the GroupNorm-in launches most of the shape's gain.  Spreading
  // those 40 over more gaps made the compiler spill to scratch inside the K loop, whose reloads wait with vmcnt(0).)
  auto mma = [&](int cc, int t) {
    __builtin_amdgcn_s_setprio(1);
    // (unconditional on the last half-slice too: it then rewrites the re-read copy in the buffer nobody reads any more)
    const bool xf = gn_in && t >= 3 && t < 3 + NPIECE;
    if (xf) {  // the five LDS reads go out first; their latency hides behind the first eight MFMAs
      gn_read(t - 3, cc + 1);
      sched_fence();
    }
    int n = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);  // D^T
        if (xf && n == 7) {
          sched_fence();
          gn_finish(t - 3, cc + 1);  // ~30 VALU + one LDS write, spread between the following MFMAs
        }
        ++n;
      }
    if (xf) {
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // one MFMA
        __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);  // up to two VALU
      }
    }
    __builtin_amdgcn_s_setprio(0);
  };

  // Tell the compiler's waitcnt pass that the fragments are complete HERE (it is called right after the explicit lgkmcnt(0)
  // of the L segment): otherwise it inserts its own s_waitcnt lgkmcnt(0) at the first MFMA of the M segment, behind the
  // GroupNorm transform's LDS reads issued there, and their latency is exposed again.
  auto frags_ready = [&]() {
    asm volatile("" ::"v"(fa[0]), "v"(fa[1]), "v"(fa[2]), "v"(fa[3]), "v"(fa[4]), "v"(fa[5]), "v"(fa[6]), "v"(fa[7]), "v"(fb[0]),
                 "v"(fb[1]), "v"(fb[2]), "v"(fb[3]));
  };

  // ---- prologue: halo of half-slice 0 and the weights of phases 0..2 ---------------------------------------------
#pragma unroll
  for (int g = 0; g < NPIECE; ++g) issue_halo(g, 0);
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    issue_w(t, 0, c0 * 9 + t);
    issue_w(t, 1, c0 * 9 + t);
  }
  if (gn_in) {  // (a, b) of both patches' segments -> LDS (plain loads: issued after the DMA queue, waited below)
    // stored per channel PAIR as (a0, a1, b0, b1): the transform is then one packed FMA per bf16 pair
    for (int idx = tid; idx < Cin; idx += PNT) {
      const int pch = idx >= Cin / 2 ? 1 : 0, ch = (idx - pch * (Cin / 2)) * 2;
      const int seg = pch ? tl1.x : tl0.x;
      const float2 c0v = a.gn_coef[(size_t)seg * a.in_ld + ch], c1v = a.gn_coef[(size_t)seg * a.in_ld + ch + 1];
      *reinterpret_cast<float4*>(smem + COEF_OFF + (pch * Cin + ch) * 8) = make_float4(c0v.x, c1v.x, c0v.y, c1v.y);
    }
  }
  wait_vmcnt<4>();  // halo + phase 0 landed (phases 1, 2 in flight)
  if (gn_in) {
    wait_lgkmcnt0();
    fenced_barrier();  // the coefficient table is complete for every wave
#pragma unroll
    for (int g = 0; g < NPIECE; ++g) gn_piece(g, 0);
    wait_lgkmcnt0();
  }
  fenced_barrier();  // B_0

  // vmcnt immediates: a wave needs its loads of phase q+1 (issued in L(q-2)) landed before B_{2q+2}; the loads issued after
  // them are the groups of L(q-1) and L(q).  Row 0 waits at the end of M(q) (seg 2q+1), row 1 at the end of L(q) (seg 2q+1).
#define HP_PHASE0(t)                       \
  ldfrag(cc, t);                           \
  sched_fence();                           \
  issue_next(cc, t);                       \
  wait_lgkmcnt0();                         \
  if (GNIN) frags_ready();                 \
  fenced_barrier();                        \
  mma(cc, t);                              \
  wait_vmcnt<nload((t) - 1) + nload(t)>(); \
  fenced_barrier();
#define HP_PHASE1(t)                       \
  ldfrag(cc, t);                           \
  sched_fence();                           \
  issue_next(cc, t);                       \
  wait_vmcnt<nload((t) - 1) + nload(t)>(); \
  wait_lgkmcnt0();                         \
  if (GNIN) frags_ready();                 \
  fenced_barrier();                        \
  mma(cc, t);                              \
  fenced_barrier();

  if (wm == 0) {
    for (int cc = 0; cc < ncc; ++cc) {
      HP_PHASE0(0) HP_PHASE0(1) HP_PHASE0(2) HP_PHASE0(3) HP_PHASE0(4) HP_PHASE0(5) HP_PHASE0(6) HP_PHASE0(7) HP_PHASE0(8)
    }
    fenced_barrier();
  } else {
    fenced_barrier();  // the stagger
    for (int cc = 0; cc < ncc; ++cc) {
      HP_PHASE1(0) HP_PHASE1(1) HP_PHASE1(2) HP_PHASE1(3) HP_PHASE1(4) HP_PHASE1(5) HP_PHASE1(6) HP_PHASE1(7) HP_PHASE1(8)
    }
  }
  wait_vmcnt<0>();  // the zero-page tail loads must not land in the epilogue tile
  __syncthreads();

  // ---- fused epilogue: per patch two 64-row passes through an fp32 LDS tile ---------------------------------------
  float* const sC = reinterpret_cast<float*>(smem);
  bf16_t* __restrict__ out = reinterpret_cast<bf16_t*>(a.out);
  const int c8 = tid & 31, rr = tid >> 5;
  const int n0 = nt * 256 + c8 * 8;
  float sc[8], sh[8];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float4 s4v = a.scale ? reinterpret_cast<const float4*>(a.scale + n0)[h] : make_float4(1.f, 1.f, 1.f, 1.f);
    const float4 b4v = a.shift ? reinterpret_cast<const float4*>(a.shift + n0)[h] : make_float4(0.f, 0.f, 0.f, 0.f);
    sc[4 * h] = s4v.x; sc[4 * h + 1] = s4v.y; sc[4 * h + 2] = s4v.z; sc[4 * h + 3] = s4v.w;
    sh[4 * h] = b4v.x; sh[4 * h + 1] = b4v.y; sh[4 * h + 2] = b4v.z; sh[4 * h + 3] = b4v.w;
  }
  const bool relu = a.relu_nch > 0;
#pragma unroll
  for (int pp = 0; pp < 2; ++pp) {  // patch
    const SegDesc& sp = pp ? sd1 : sd0;
    const int ty = pp ? tl1.y : tl0.y;
    const int oy0 = ty >> 16, ox0 = ty & 0xffff;
    const int PW = sp.pw, NPOS = sp.ph * sp.pw;
    bf16_t* __restrict__ outn = out + (size_t)sp.out_row0 * a.out_ld + n0;
    // GroupNorm partial sums of this patch about a pivot every lane of a group shares, so that lanes and waves merge by plain
    // additions: the conv bias of the group's first channel (what makes |mean| >> sigma in practice) -- unless the patch's first
    // position says the group sits far from it (a DC component the eight channels share): then the mean of that position's eight
    // values.  The one-pass M2 = S2 - S1^2 / N loses (mean - pivot)^2 / sigma^2 of its fp32 precision: 1e-4 relative at 64 sigma.
    // (The sampled position is one of the patch's 128: even an outlier there lies within sqrt(128) patch-sigma of the patch mean.)
    float gn_n = 0.f, gn_s1 = 0.f, gn_s2 = 0.f;
    float gn_pv = sh[0];
#pragma unroll
    for (int hp = 0; hp < 2; ++hp) {  // 64-row half of the patch
      if (pp + hp > 0) lds_barrier();
      if (wm == pp) {  // 16x16x32 accumulator layout: position 16 i + l15, channels 16 j + 4 lq .. + 3
#pragma unroll
        for (int ii = 0; ii < 4; ++ii)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const f32x4& c = acc[4 * hp + ii][j];
            *reinterpret_cast<float4*>(sC + (ii * 16 + l15) * SCP + wn * 64 + j * 16 + 4 * lq) = make_float4(c[0], c[1], c[2], c[3]);
          }
      }
      lds_barrier();
      if (hp == 0 && a.gn_partial) {  // row 0 of the patch, read by all sixteen row-lanes of the group (an LDS broadcast)
        const float4 lo = *reinterpret_cast<const float4*>(sC + c8 * 8);
        const float4 hi = *reinterpret_cast<const float4*>(sC + c8 * 8 + 4);
        float v0[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        float vmin = 3.4e38f, vmax = -3.4e38f, vsum = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float t = v0[e] * sc[e] + sh[e];
          if (relu) t = t > 0.f ? t : 0.f;
          vmin = fminf(vmin, t); vmax = fmaxf(vmax, t); vsum += t;
        }
        const float m0 = vsum * 0.125f;
        if (fabsf(m0 - gn_pv) > 4.f * (vmax - vmin)) gn_pv = m0;  // further off than four times the spread of the eight values
      }
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int rl = rr + 16 * it;
        const int m = hp * 64 + rl;
        const int my = (int)(((unsigned)m * sp.inv_pw) >> 16);
        const int oy = oy0 + my, ox = ox0 + (m - my * PW);
        if (m < NPOS && oy < sp.out_H && ox < sp.out_W) {
          float v[8];
          const float4 lo = *reinterpret_cast<const float4*>(sC + rl * SCP + c8 * 8);
          const float4 hi = *reinterpret_cast<const float4*>(sC + rl * SCP + c8 * 8 + 4);
          v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = v[e] * sc[e] + sh[e];
          if (relu) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
          }
          if (a.gn_partial) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float d = v[e] - gn_pv; gn_s1 += d; gn_s2 = fmaf(d, d, gn_s2); }
            gn_n += 8.f;
          }
          store8<bf16_t>(outn + (size_t)(oy * sp.out_W + ox) * a.out_ld, v);
        }
      }
    }
    if (a.gn_partial) {  // one (n, mean, M2) partial per patch and 8-channel group, merged in a fixed order
      gn_n += __shfl_xor(gn_n, 32);  // lanes c8 and c8 + 32 of a wave hold the same group (rows rr, rr + 1)
      gn_s1 += __shfl_xor(gn_s1, 32);
      gn_s2 += __shfl_xor(gn_s2, 32);
      lds_barrier();
      float* red = sC;  // [8 waves][32 groups][3]
      if (lane < 32) {
        red[(wave * 32 + c8) * 3 + 0] = gn_n;
        red[(wave * 32 + c8) * 3 + 1] = gn_s1;
        red[(wave * 32 + c8) * 3 + 2] = gn_s2;
      }
      lds_barrier();
      if (tid < 32) {
        float N = 0.f, S1 = 0.f, S2 = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) {
          N += red[(w * 32 + c8) * 3 + 0]; S1 += red[(w * 32 + c8) * 3 + 1]; S2 += red[(w * 32 + c8) * 3 + 2];
        }
        const float inv_n = N > 0.f ? 1.f / N : 0.f;
        const float m2 = S2 - S1 * S1 * inv_n;
        float* gp = a.gn_partial + ((size_t)(2 * mt + pp) * (a.Cout >> 3) + (n0 >> 3)) * 3;
        gp[0] = N; gp[1] = gn_pv + S1 * inv_n; gp[2] = m2 > 0.f ? m2 : 0.f;
      }
    }
  }
}

// [Cout][3][3][Cin] bf16 (conv_igemm layout) -> [Cout / 256][Cin / 32][9][256 rows][4 slots][8] with the stage swizzle applied
// (slot s of row r holds chunk s ^ sw(r), "LDS images" above)
__global__ void hpipe_pack_weights_kernel(const bf16_t* __restrict__ w, bf16_t* __restrict__ out, int Cout, int Cin) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // one 16-byte chunk
  const size_t nchunks = (size_t)Cout * 9 * Cin / 8;
  if (i >= nchunks) return;
  const int ncc = Cin >> 5;
  const int s = (int)(i & 3), r = (int)((i >> 2) & 255);
  const size_t blk = i >> 10;
  const int t = (int)(blk % 9), c = (int)((blk / 9) % ncc), nt = (int)(blk / (9 * (size_t)ncc));
  const int chunk = s ^ (((r >> 2) & 1) << 1);
  const uint4 v = *reinterpret_cast<const uint4*>(w + ((size_t)(nt * 256 + r) * 9 + t) * Cin + c * 32 + chunk * 8);
  *reinterpret_cast<uint4*>(out + i * 8) = v;
}

int launch_hpipe_pack_weights(const void* w, void* out, int Cout, int Cin, hipStream_t s) {
  const size_t nchunks = (size_t)Cout * 9 * Cin / 8;
  hipLaunchKernelGGL(hpipe_pack_weights_kernel, dim3((unsigned)((nchunks + 255) / 256)), dim3(256), 0, s, (const bf16_t*)w, (bf16_t*)out, Cout, Cin);
  return (int)hipGetLastError();
}

bool conv_hpipe_ok(DType dt, bool out_f32, const ConvArgs& a) {
  if (a.gn_coef && a.Cin > COEF_MAX_CIN) return false;
  return dt == DT_BF16 && !out_f32 && !a.stem && !a.in2 && a.res_mode == 0 && a.mul_nch == 0 && a.KH == 3 && a.KW == 3 &&
         a.stride == 1 && a.pad == 1 && (a.relu_nch == 0 || a.relu_nch >= a.Cout) && a.Cout % 256 == 0 && a.Cin % 32 == 0 &&
         a.Cin >= 32 && a.ss_padded && (a.out_ld & 7) == 0 && a.zeros != nullptr;
}

int launch_conv_hpipe(const ConvArgs& a, hipStream_t s) {
  static PerDeviceOnce once;
  if (!once.run(current_device(), [] {
        return hipFuncSetAttribute((const void*)conv_hpipe_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES) == hipSuccess &&
               hipFuncSetAttribute((const void*)conv_hpipe_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES) == hipSuccess;
      }))
    return -7;
  const int chunk = (a.n_mtiles + 7) / 8;
  const int grid = 8 * chunk * a.n_ntiles;
  if (a.gn_coef) hipLaunchKernelGGL(conv_hpipe_kernel<true>, dim3(grid), dim3(PNT), LDS_BYTES, s, a);
  else hipLaunchKernelGGL(conv_hpipe_kernel<false>, dim3(grid), dim3(PNT), LDS_BYTES, s, a);
  return (int)hipGetLastError();
}

}  // namespace sylph
