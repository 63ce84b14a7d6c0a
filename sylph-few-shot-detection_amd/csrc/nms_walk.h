// The greedy NMS walk in chunks of 64 score-sorted boxes, once: for nms_kernel (detect.hip), merge_views_kernel (merge_views.hip),
// merge_large_nms_kernel and both rules of stitch_walk_kernel (merge_views_large.hip).  A chunk is one wave's ballot:
//   - the boxes kept in earlier chunks suppress through per-wave ballots (the caller's loop, or walk_kept_groups below),
//   - walk_fill_matrix: the 64 x 64 bits "box i suppresses box j > i" inside the chunk, four pairs per thread of a 1024-thread block,
//   - walk_resolve: wave 0 walks the chunk serially: a box is kept iff no kept box before it suppresses it,
//   - walk_select_kth / walk_emits: the post-NMS keep (the first K kept boxes and every later one whose score ties the K-th).
// block_walk is the whole walk of a pool one block holds; the segment_* pieces and walk_kept_groups serve the walks over a caller's
// workspace.  Every including unit is built without FMA contraction: the overlap arithmetic (merge_math.h) is pinned bit for bit.
#pragma once
#include "common.h"
#include "kernels.h"
#include "merge_math.h"

namespace sylph {

constexpr unsigned long long KEY_NONE = ~0ull;  // the high word of a sort key that holds no row (merge_views_large.hip)

// s_d [64][2], cleared before: bit j of row i <- pred(i, j) for j > i.  Thread t takes i = t >> 4 and j = 4 (t & 15) .. + 3
template <class Pred>
__device__ __forceinline__ void walk_fill_matrix(unsigned (*s_d)[2], int t, Pred pred) {
  const int i = t >> 4, jq = t & 15;
  unsigned bits = 0u;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int j = 4 * jq + e;
    if (j > i && pred(i, j)) bits |= 1u << (j & 31);
  }
  if (bits) atomicOr(&s_d[i][jq >> 3], bits);
}

// wave 0.  cur: the lanes that cannot be kept (suppressed from outside the chunk, or past the end) -> the lanes kept.  INK: *ink <- the
// first kept lane whose row holds this lane's bit, -1 without one
template <bool INK>
__device__ __forceinline__ unsigned long long walk_resolve(unsigned long long cur, const unsigned (*s_d)[2], int lane, int* ink) {
  const unsigned long long d = ((unsigned long long)s_d[lane][1] << 32) | (unsigned long long)s_d[lane][0];
  unsigned long long keptmask = 0ull;
  int first = -1;
  for (int b = 0; b < 64; ++b) {
    const unsigned long long db = merge_shfl_u64(d, b);
    if (!((cur >> b) & 1ull)) {
      keptmask |= 1ull << b;
      cur |= db;
      if (INK && first < 0 && ((db >> lane) & 1ull)) first = b;
    }
  }
  if (INK) *ink = first;
  return keptmask;
}

// wave 0, once per walk: when this chunk holds the K-th kept box, kth <- that lane's `mine` (its score, or an order word of it)
template <class T>
__device__ __forceinline__ void walk_select_kth(int K, int kept_total, unsigned long long keptmask, bool is_kept, int rank, T mine, T* kth,
                                                bool* have_kth) {
  if (K > 0 && !*have_kth && kept_total + __popcll(keptmask) >= K) {
    const unsigned long long sel = __ballot(is_kept && rank == K - 1);
    *kth = __shfl(mine, __ffsll((long long)sel) - 1);
    *have_kth = true;
  }
}

// rule 5 for a kept box (kth is set once a rank reaches K)
__device__ __forceinline__ bool walk_emits(int K, int rank, float score, float kth) { return K <= 0 || rank < K || score >= kth; }

struct BlockWalkLds {
  // the chunk's lanes that a box kept in an earlier chunk suppresses.  The waves OR their ballots into this one word: sixteen words that
  // wave 0 reads back in one batch held 32 VGPRs there and set the register count of both kernels (profiles/nms_walk_core.txt)
  unsigned long long sup;
  unsigned d[64][2];  // suppression bits inside the chunk: row i = the boxes of the chunk that box i suppresses
  float4 box4[64];
  int cls4[64];
  int kept_total, stop;
};

// The walk of a score-sorted pool of n boxes that one 1024-thread block holds, class-aware, with rule 5's keep; blockIdx.x is the output
// slot.  It begins with a barrier: what the caller left in LDS is there.  kept_pos [n] (LDS) receives the pool positions of the kept
// boxes.  src gives
//   box(p), cls(p), score(p)            of pool position p, for the chunk's load and for a kept position alike
//   shape(b)                            a kept box on its way out: may rewrite it, false drops it
//   write(o, p, b, score, cls)          output row o <- the box of pool position p
// Wave 0 returns the number of boxes it emitted (the caller clamps it to max_out) and, per lane, whether its box found no row.
// A walk with K > 0 stops at the first chunk whose best score is below the K-th kept score; have_kth rather than a negative kth marks
// "not yet", so scores of any sign walk alike (decode scores lie above its 0.05 threshold, where a kth < 0 sentinel meant the same).
template <class Src>
__device__ __forceinline__ int block_walk(BlockWalkLds& w, unsigned short* kept_pos, unsigned n, float thr, int K, int max_out, const Src& src,
                                          bool* truncated_out) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nw = (int)((n + 63) / 64);
  const bool nms_on = thr > 0.f;
  int kept_total = 0, nout = 0;  // wave 0 keeps the running state; kept_total is mirrored in LDS for the other waves
  float kth = 0.f;
  bool have_kth = false, truncated = false;
  if (t == 0) { w.kept_total = 0; w.stop = 0; }
  __syncthreads();
  for (int c = 0; c < nw; ++c) {
    const unsigned b0 = c * 64;
    // the chunk's boxes -> LDS (wave 0), suppression words cleared
    if (wave == 0) {
      const unsigned bi = b0 + lane;
      if (bi < n) {
        w.box4[lane] = src.box(bi);
        w.cls4[lane] = src.cls(bi);
      } else {
        w.box4[lane] = make_float4(0.f, 0.f, 0.f, 0.f);
        w.cls4[lane] = -1 - lane;  // matches nothing
      }
      w.d[lane][0] = 0u; w.d[lane][1] = 0u;
      if (lane == 0) w.sup = 0ull;
    }
    __syncthreads();
    const int ktot = w.kept_total;
    const float4 mb = w.box4[lane];
    const int mc = w.cls4[lane];
    bool sup = false;
    if (nms_on) {
      // against the kept boxes of earlier chunks (kept box = the earlier, higher-scored one: "i" of the pair): box lane against every
      // 16th kept box, class first; the kept box is one broadcast 16-byte load per wave
      for (int k = wave; k < ktot; k += 16) {
        const unsigned kp = kept_pos[k];
        if (src.cls(kp) != mc) continue;
        const float4 kb = src.box(kp);
        const float karea = (kb.z - kb.x) * (kb.w - kb.y);
        sup = sup || merge_overlap(kb.x, kb.y, kb.z, kb.w, karea, mb, thr);
      }
      const float4 ib = w.box4[t >> 4];
      const int ic = w.cls4[t >> 4];
      const float iarea = (ib.z - ib.x) * (ib.w - ib.y);
      walk_fill_matrix(w.d, t, [&](int, int j) { return w.cls4[j] == ic && merge_overlap(ib.x, ib.y, ib.z, ib.w, iarea, w.box4[j], thr); });
    }
    const unsigned long long part = __ballot(sup);
    if (lane == 0 && part) atomicOr(&w.sup, part);
    __syncthreads();
    if (wave == 0) {
      const unsigned bi = b0 + lane;
      const bool valid = bi < n;
      unsigned long long cur = w.sup;
      if (n - b0 < 64u) cur |= ~0ull << (n - b0);
      const unsigned long long keptmask = walk_resolve<false>(cur, w.d, lane, nullptr);
      const int nk = __popcll(keptmask);
      const bool is_kept = (keptmask >> lane) & 1ull;
      const int rank = kept_total + __popcll(keptmask & ((1ull << lane) - 1ull));
      if (is_kept) kept_pos[rank] = (unsigned short)bi;
      const float score = valid ? src.score(bi) : 0.f;
      walk_select_kth(K, kept_total, keptmask, is_kept, rank, score, &kth, &have_kth);
      bool emit = is_kept && walk_emits(K, rank, score, kth);
      float4 ob = mb;
      if (emit) emit = src.shape(ob);
      const unsigned long long em = __ballot(emit);
      const int slot = nout + __popcll(em & ((1ull << lane) - 1ull));
      if (emit) {
        if (slot < max_out) src.write((size_t)blockIdx.x * max_out + slot, bi, ob, score, mc);
        else truncated = true;
      }
      nout += __popcll(em);
      kept_total += nk;
      bool stop = false;
      if (K > 0 && kept_total >= K && c + 1 < nw) stop = src.score(b0 + 64) < kth;  // nothing below the K-th kept score can be emitted any more
      if (lane == 0) { w.kept_total = kept_total; w.stop = stop ? 1 : 0; }
    }
    __syncthreads();
    if (w.stop) break;
  }
  *truncated_out = truncated;
  return nout;
}

// ---- the walks over a caller's workspace (merge_views_large.hip): keys sorted by (source, class, score descending), a block of 64 sorted
// positions from p0 walks every (source, class) segment that starts among them

// -> the bits of the positions p0 + lane at which a segment starts (P is a multiple of 64).  Ends with a barrier
__device__ __forceinline__ unsigned long long segment_starts(const ulonglong2* __restrict__ keys, unsigned p0, unsigned long long* s_starts) {
  if (threadIdx.x < 64) {
    const unsigned p = p0 + threadIdx.x;
    const unsigned long long hi = keys[p].x;
    const bool start = hi != KEY_NONE && (p == 0 || keys[p - 1].x != hi);
    const unsigned long long m = __ballot(start);
    if (threadIdx.x == 0) *s_starts = m;
  }
  __syncthreads();
  return *s_starts;
}

// wave 0: sorted position pos of the segment whose keys' high word is seg_hi -> box4[lane] in source coordinates (zeros past the segment's
// end), the lane's matrix row cleared, *s_valid the lanes inside the segment (a segment is a run of the sorted keys: a chunk's first
// ones).  Returns whether the lane is inside; *key_lo, *bx: the key's low word and the box, zeros past the end
__device__ __forceinline__ bool segment_chunk_load(const ulonglong2* __restrict__ keys, unsigned P, unsigned long long pos,
                                                   unsigned long long seg_hi, const float* __restrict__ boxes,
                                                   const MergeView* __restrict__ views, int max_in, int lane, float4* box4, unsigned (*s_d)[2],
                                                   unsigned long long* s_valid, unsigned long long* key_lo, float4* bx) {
  bool valid = false;
  *key_lo = 0ull;
  *bx = make_float4(0.f, 0.f, 0.f, 0.f);
  if (pos < P) {
    const ulonglong2 k = keys[pos];
    if (k.x == seg_hi) {
      valid = true;
      *key_lo = k.y;
      *bx = merge_source_box(boxes, views, (unsigned)(k.y & 0xffffffffull), (unsigned)max_in);
    }
  }
  box4[lane] = *bx;
  s_d[lane][0] = 0u; s_d[lane][1] = 0u;
  const unsigned long long vm = __ballot(valid);
  if (lane == 0) *s_valid = vm;
  return valid;
}

// The first `count` entries of a segment's kept list against the lane's box mb, in groups of 64, a group per wave of the 16.  Entries
// below MERGE_LARGE_KEPT_LDS are read from s_list; a group beyond comes in from g_list (the segment's part of the workspace) with one
// coalesced load into the wave's 64 entries of s_stage and is then read like the LDS list, one box for all lanes (MERGE_LARGE_KEPT_LDS is
// a multiple of 64: a group is on one side).  An entry that no lane's box intersects is done after the intersection -- no test of any
// walk passes at inter = 0 -- so a division runs only for the few kept boxes near the chunk's: body(rank, box, meta) sees the others.
// META: a word per entry (s_meta / g_meta, staged in s_stagem) goes along.  PREFETCH: the next entry is in flight under the body
template <bool PREFETCH, bool META, class Body>
__device__ __forceinline__ void walk_kept_groups(int count, int lane, int wave, float4 mb, const float4* s_list, const float4* g_list,
                                                 float4* s_stage, const unsigned* s_meta, const unsigned* g_meta, unsigned* s_stagem, Body body) {
  for (int base = wave * 64; base < count; base += 16 * 64) {
    const int cnt = count - base < 64 ? count - base : 64;
    const float4* grp = s_list + base;
    const unsigned* gm = META ? s_meta + base : nullptr;
    if (base >= MERGE_LARGE_KEPT_LDS) {
      if (lane < cnt) {
        s_stage[wave * 64 + lane] = g_list[base + lane];
        if (META) s_stagem[wave * 64 + lane] = g_meta[base + lane];
      }
      grp = s_stage + wave * 64;
      if (META) gm = s_stagem + wave * 64;
    }
    float4 next = grp[0];
    for (int j = 0; j < cnt; ++j) {
      float4 kb;
      if (PREFETCH) {
        kb = next;
        if (j + 1 < cnt) next = grp[j + 1];
      } else {
        kb = grp[j];
      }
      const float iw = fmaxf(0.f, fminf(kb.z, mb.z) - fmaxf(kb.x, mb.x)), ih = fmaxf(0.f, fminf(kb.w, mb.w) - fmaxf(kb.y, mb.y));
      if (__any(iw * ih > 0.f)) body(base + j, kb, META ? gm[j] : 0u);
    }
  }
}

}  // namespace sylph
