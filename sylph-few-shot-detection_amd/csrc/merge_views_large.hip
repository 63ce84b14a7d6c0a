// Merge of the detections of several views of one source with no LDS-sized pool limit: gfx950.  The rules and the result are those of
// merge_views_kernel (merge_views.hip; include/sylph_hip.h above sylph_merge_views), bit for bit; the pool lives in a caller's workspace
// and class-aware NMS runs per (source, class) segment.  The launches of one call, all on one stream, no atomics, nothing kept:
//   1  keys: every row g = view * max_in + row of the [n_views][max_in] buffers becomes a 128-bit key
//        hi = source << 32 | class bits,  lo = ~(ordered score bits) << 32 | g      (rows beyond a view's count and the padding: all ones)
//   2  bitonic sort, ascending, over P = the power of two >= n_views * max_in (at least one tile): MERGE_LARGE_SORT_TILE keys per block
//      in LDS for the strides below a tile, one compare-exchange per thread in global memory for the strides above.  The keys are
//      unique, so the order is (source, class, score descending, view, row) whatever the network does
//   3  NMS: the block of 64 sorted positions walks every segment that STARTS among them (most blocks find none and leave), in chunks of
//      MERGE_LARGE_CHUNK = 64 boxes with the pieces of nms_walk.h that step 4 of merge_views_kernel is made of: ballots against the boxes
//      kept in earlier chunks (walk_kept_groups), a 64 x 64 bit matrix inside the chunk (walk_fill_matrix, on IoU alone: a segment is one
//      class), a serial resolve in wave 0 (walk_resolve).  The first MERGE_LARGE_KEPT_LDS kept boxes of a segment stay in LDS, later
//      ones spill to the workspace at (segment start + rank): a segment keeps at most as many boxes as it holds.  The waves take the
//      kept boxes in groups of 64 and skip the division for a box that meets none of the chunk's.  With K > 0 a segment stops once it
//      has kept K boxes and the scores have fallen below its K-th: rule 5 cannot emit what lies behind
//   4  keys again: hi = source for a kept row, all ones for the others; the same sort -> per source its kept rows in rule-3 order
//   5  the bounds of every source's run, then emit: with the rows in score order rule 5 keeps a PREFIX (rank < K or score >= the K-th),
//      so every thread decides from its own row and its neighbour's; the thread of the last emitted row writes the count
#include "common.h"
#include "kernels.h"
#include "nms_walk.h"

namespace sylph {

namespace {

constexpr int TILE = MERGE_LARGE_SORT_TILE, CHUNK = MERGE_LARGE_CHUNK, KEPT_LDS = MERGE_LARGE_KEPT_LDS;
static_assert(CHUNK == 64 && KEPT_LDS % 64 == 0, "one chunk is one wave's ballot; the kept boxes are compared in groups of 64");
static_assert(TILE == 2048, "the tile sort gives each of its 1024 threads one pair");

__device__ __forceinline__ bool key_less(ulonglong2 a, ulonglong2 b) { return a.x < b.x || (a.x == b.x && a.y < b.y); }

// 1: a count outside [0, max_in] is clamped, as merge_views_kernel does
__global__ __launch_bounds__(256) void merge_large_keys_kernel(ulonglong2* __restrict__ keys, unsigned P, unsigned n_rows, int max_in,
                                                               const MergeView* __restrict__ views, const float* __restrict__ scores,
                                                               const int* __restrict__ classes, const int* __restrict__ counts) {
  const unsigned g = blockIdx.x * 256u + threadIdx.x;
  if (g >= P) return;
  ulonglong2 key = make_ulonglong2(KEY_NONE, KEY_NONE);
  if (g < n_rows) {
    const unsigned v = g / (unsigned)max_in, r = g % (unsigned)max_in;
    const int cn = counts[v];
    const unsigned rows = cn < 0 ? 0u : (cn > max_in ? (unsigned)max_in : (unsigned)cn);
    if (r < rows) {
      key.x = ((unsigned long long)(unsigned)views[v].src << 32) | (unsigned long long)(unsigned)classes[g];
      key.y = ((unsigned long long)(~merge_score_key(scores[g])) << 32) | (unsigned long long)g;
    }
  }
  keys[g] = key;
}

// 2: the steps of the bitonic network whose stride is below a tile, for the sizes size_first ... size_last (powers of two; a size above
// the tile starts at stride TILE / 2: its larger strides were merge_large_sort_step_kernel's)
__global__ __launch_bounds__(1024) void merge_large_sort_tile_kernel(ulonglong2* __restrict__ keys, unsigned size_first, unsigned size_last) {
  __shared__ unsigned long long s_hi[TILE], s_lo[TILE];
  const unsigned t = threadIdx.x, base = blockIdx.x * (unsigned)TILE;
  for (unsigned i = t; i < (unsigned)TILE; i += 1024) {
    const ulonglong2 k = keys[base + i];
    s_hi[i] = k.x; s_lo[i] = k.y;
  }
  __syncthreads();
  for (unsigned size = size_first; size <= size_last && size != 0; size <<= 1) {
    unsigned stride = size >> 1;
    if (stride > (unsigned)TILE / 2) stride = TILE / 2;
    for (; stride > 0; stride >>= 1) {
      const unsigned lo = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), hi = lo + stride;
      const bool asc = ((base + lo) & size) == 0;
      const ulonglong2 a = make_ulonglong2(s_hi[lo], s_lo[lo]), b = make_ulonglong2(s_hi[hi], s_lo[hi]);
      if (key_less(b, a) == asc) {
        s_hi[lo] = b.x; s_lo[lo] = b.y;
        s_hi[hi] = a.x; s_lo[hi] = a.y;
      }
      __syncthreads();
    }
  }
  for (unsigned i = t; i < (unsigned)TILE; i += 1024) keys[base + i] = make_ulonglong2(s_hi[i], s_lo[i]);
}

// 2: one step of a stride of at least a tile: P / 2 threads, one pair each
__global__ __launch_bounds__(256) void merge_large_sort_step_kernel(ulonglong2* __restrict__ keys, unsigned P, unsigned size, unsigned stride) {
  const unsigned u = blockIdx.x * 256u + threadIdx.x;
  if (u >= (P >> 1)) return;
  const unsigned lo = ((u & ~(stride - 1)) << 1) | (u & (stride - 1)), hi = lo + stride;
  const bool asc = (lo & size) == 0;
  const ulonglong2 a = keys[lo], b = keys[hi];
  if (key_less(b, a) == asc) { keys[lo] = b; keys[hi] = a; }
}

// 3: see the head of the file.  kept [n_rows] (cleared before): set for every sorted position whose row is kept.  K > 0: a segment
// that has kept K boxes stops at the first chunk that begins below its K-th kept score -- the source's K-th kept score is no lower,
// so rule 5 emits none of the rows behind (the early stop of merge_views_kernel, per segment); they stay unkept
__global__ __launch_bounds__(1024) void merge_large_nms_kernel(const ulonglong2* __restrict__ keys, unsigned P, const MergeView* __restrict__ views,
                                                               int max_in, const float* __restrict__ boxes, float thr, int K, float4* kbox,
                                                               unsigned char* __restrict__ kept) {
  __shared__ float4 s_kept[KEPT_LDS];
  __shared__ float4 s_stage[16][64];  // per wave: the group of spilled kept boxes it is comparing against
  __shared__ unsigned long long s_part[16];
  __shared__ unsigned s_d[64][2];
  __shared__ float4 s_box4[64];
  __shared__ unsigned long long s_starts, s_valid;
  __shared__ int s_kept_total, s_last;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const unsigned p0 = blockIdx.x * 64u;
  unsigned long long starts = segment_starts(keys, p0, &s_starts);
  while (starts) {
    const unsigned seg0 = p0 + (unsigned)(__ffsll((long long)starts) - 1);
    starts &= starts - 1;
    const unsigned long long seg_hi = keys[seg0].x;
    int kept_total = 0;  // wave 0 keeps the running state; mirrored in LDS for the other waves
    unsigned ord = 0u, kth_ord = 0u;  // ~(ordered score bits) of the lane's row and of the segment's K-th kept row: ascending = score descending
    bool have_kth = false;
    if (t == 0) s_kept_total = 0;
    for (unsigned c = 0;; ++c) {
      const unsigned long long pos = (unsigned long long)seg0 + 64ull * c + (unsigned)lane;
      if (wave == 0) {
        unsigned long long lo;
        float4 bx;
        segment_chunk_load(keys, P, pos, seg_hi, boxes, views, max_in, lane, s_box4, s_d, &s_valid, &lo, &bx);
        ord = (unsigned)(lo >> 32);
      }
      __syncthreads();
      const int ktot = s_kept_total;
      const unsigned long long vmask = s_valid;
      const float4 mb = s_box4[lane];
      bool sup = false;
      walk_kept_groups<true, false>(ktot, lane, wave, mb, s_kept, kbox + seg0, &s_stage[0][0], nullptr, nullptr, nullptr,
                                    [&](int, float4 kb, unsigned) {
                                      const float karea = (kb.z - kb.x) * (kb.w - kb.y);
                                      sup = sup || merge_overlap(kb.x, kb.y, kb.z, kb.w, karea, mb, thr);
                                    });
      {
        const float4 ib = s_box4[t >> 4];
        const float iarea = (ib.z - ib.x) * (ib.w - ib.y);
        walk_fill_matrix(s_d, t, [&](int, int j) { return merge_overlap(ib.x, ib.y, ib.z, ib.w, iarea, s_box4[j], thr); });
      }
      const unsigned long long part = __ballot(sup);
      if (lane == 0) s_part[wave] = part;
      __syncthreads();
      if (wave == 0) {
        unsigned long long cur = ~vmask;  // the lanes past the segment's end are never kept
#pragma unroll
        for (int w = 0; w < 16; ++w) cur |= s_part[w];
        const unsigned long long keptmask = walk_resolve<false>(cur, s_d, lane, nullptr);
        const bool is_kept = (keptmask >> lane) & 1ull;
        const int rank = kept_total + __popcll(keptmask & ((1ull << lane) - 1ull));
        if (is_kept) {
          if (rank < KEPT_LDS) s_kept[rank] = mb;
          else kbox[(size_t)seg0 + rank] = mb;
        }
        if (is_kept) kept[pos] = 1;
        walk_select_kth(K, kept_total, keptmask, is_kept, rank, ord, &kth_ord, &have_kth);
        kept_total += __popcll(keptmask);
        bool last = vmask != ~0ull;
        if (!last && have_kth && lane == 0) {  // does the next chunk begin below the K-th kept score?
          const unsigned long long np = (unsigned long long)seg0 + 64ull * (c + 1);
          if (np < P) {
            const ulonglong2 nk = keys[np];
            last = nk.x == seg_hi && (unsigned)(nk.y >> 32) > kth_ord;
          }
        }
        if (lane == 0) { s_kept_total = kept_total; s_last = last ? 1 : 0; }
      }
      __syncthreads();
      if (s_last) break;
    }
  }
}

// 4: the keys of the second sort: hi = source for a row that stays.  The large merge: sorted position i stays when kept[i] is set, or
// nms_on == 0 (thr <= 0: every row stays, the NMS kernel did not run).  STITCH: a row stays when cnt [n_rows], indexed by INPUT row, holds
// its 1 + what the survivor absorbed and not 0
template <bool STITCH>
__global__ __launch_bounds__(256) void merge_large_rekey_kernel(ulonglong2* __restrict__ keys, unsigned P, const unsigned char* __restrict__ kept,
                                                                int nms_on, const int* __restrict__ cnt) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= P) return;
  ulonglong2 k = keys[i];
  if (k.x == KEY_NONE) return;
  // (the test stays inside the if: held in a bool first, hipcc of ROCm 7 emitted a kept row's k.y as all ones on the nms_on path)
  if (STITCH ? cnt[(unsigned)(k.y & 0xffffffffull)] != 0 : (!nms_on || kept[i])) k.x >>= 32;
  else k = make_ulonglong2(KEY_NONE, KEY_NONE);
  keys[i] = k;
}

// 5: bounds [n_src][2] (cleared before: a source without a kept row keeps 0, 0): the run of every source in the sorted keys
__global__ __launch_bounds__(256) void merge_large_bounds_kernel(const ulonglong2* __restrict__ keys, unsigned P, unsigned* __restrict__ bounds) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= P) return;
  const unsigned long long hi = keys[i].x;
  if (hi == KEY_NONE) return;
  if (i == 0 || keys[i - 1].x != hi) bounds[2 * hi] = i;
  if (i + 1 == P || keys[i + 1].x != hi) bounds[2 * hi + 1] = i + 1;
}

// 5: thread j of source blockIdx.x / blocks_per_src looks at the source's j-th kept row, j <= max_out (row max_out only tells that the source is truncated).
// STITCH: the rows are the survivors, the same prefix rule on their own scores; the box is the union box ubox [n_rows] of the input row,
// out_stitched its count cnt [n_rows] (neither is touched otherwise)
template <bool STITCH>
__global__ __launch_bounds__(256) void merge_large_emit_kernel(const ulonglong2* __restrict__ keys, const unsigned* __restrict__ bounds,
                                                               const MergeView* __restrict__ views, int max_in, const float* __restrict__ boxes,
                                                               const float4* __restrict__ ubox, const int* __restrict__ cnt,
                                                               const float* __restrict__ scores, const int* __restrict__ classes, int K,
                                                               int max_out, int blocks_per_src, float* out_boxes, float* out_scores, int* out_classes, int* out_view,
                                                               int* out_row, int* out_stitched, int* out_counts, int* status) {
  const int src = blockIdx.x / blocks_per_src;
  const unsigned j = (blockIdx.x % blocks_per_src) * 256u + threadIdx.x;
  const unsigned beg = bounds[2 * src], n = bounds[2 * src + 1] - beg;
  if (n == 0) {
    if (j == 0) out_counts[src] = 0;
    return;
  }
  if (j >= n || j > (unsigned)max_out) return;
  const unsigned g = (unsigned)(keys[beg + j].y & 0xffffffffull);
  const float score = scores[g];
  const bool cut = K > 0 && n > (unsigned)K;
  const float kth = cut ? scores[(unsigned)(keys[beg + K - 1].y & 0xffffffffull)] : 0.f;
  if (cut && j >= (unsigned)K && !(score >= kth)) return;
  bool next = j + 1 < n;  // is the row behind this one emitted too?
  if (next && cut && j + 1 >= (unsigned)K) next = scores[(unsigned)(keys[beg + j + 1].y & 0xffffffffull)] >= kth;
  if (j == (unsigned)max_out) {  // (every truncated source stores the same word: no atomic)
    *status = 2;
    out_counts[src] = max_out;
    return;
  }
  const float4 b = STITCH ? ubox[g] : merge_source_box(boxes, views, g, (unsigned)max_in);
  const size_t o = (size_t)src * max_out + j;
  out_boxes[o * 4 + 0] = b.x; out_boxes[o * 4 + 1] = b.y; out_boxes[o * 4 + 2] = b.z; out_boxes[o * 4 + 3] = b.w;
  out_scores[o] = score;
  out_classes[o] = classes[g];
  out_view[o] = (int)(g / (unsigned)max_in);
  out_row[o] = (int)(g % (unsigned)max_in);
  if (STITCH) out_stitched[o] = cnt[g];
  if (!next) out_counts[src] = (int)j + 1;
}

void sort_keys(ulonglong2* keys, unsigned P, hipStream_t s) {
  const unsigned tiles = P / TILE, steps = (P / 2 + 255) / 256;
  hipLaunchKernelGGL(merge_large_sort_tile_kernel, dim3(tiles), dim3(1024), 0, s, keys, 2u, (unsigned)TILE);
  for (unsigned long long size = 2ull * TILE; size <= P; size <<= 1) {
    for (unsigned stride = (unsigned)(size >> 1); stride >= (unsigned)TILE; stride >>= 1)
      hipLaunchKernelGGL(merge_large_sort_step_kernel, dim3(steps), dim3(256), 0, s, keys, P, (unsigned)size, stride);
    hipLaunchKernelGGL(merge_large_sort_tile_kernel, dim3(tiles), dim3(1024), 0, s, keys, (unsigned)size, (unsigned)size);
  }
}

// ---- the stitching merge (sylph_stitch_views): launches 1 and 2 as above, then
//   3s  stitch_walk_kernel: per (source, class) segment, rule 4a as launch 3 walks it -- but a row remembers the LOWEST-ranked kept box
//       that matches it (its keeper), every kept box carries a cut bit, a union box U and a count next to its own box (in LDS up to
//       MERGE_LARGE_KEPT_LDS, spilled beyond), and there is no early stop: a row behind the K-th kept score can still grow an emitted box.
//       Then rule 4b over the segment's kept boxes, 64 ranks a step, against the frozen U of the earlier survivors; then every survivor
//       leaves U and 1 + its count at its INPUT row
//   4s  launches 4 and 5 in their STITCH instantiation: a row with a count survives; the same sort and bounds; the emit with U as the box
// Both rules run on the walk's pieces of nms_walk.h: the segment prologue and chunk load of launch 3, walk_kept_groups with a meta word per
// kept box and a body that records the lowest matching rank, walk_fill_matrix on stitch_match (4a) or stitch_covered (4b), and the
// walk_resolve that also names the first kept box of the chunk holding the lane's bit.
// The hull is a min / max, the counts are integers: no order of arrival can change a bit.

constexpr unsigned META_CUT = 0x80000000u, META_DROPPED = 0x40000000u, META_COUNT = 0x3fffffffu;
constexpr int NO_KEEPER = 0x7fffffff;
// dynamic LDS of stitch_walk_kernel: kept boxes | their U | the waves' staged groups (boxes) | meta | input rows | staged meta
constexpr size_t STITCH_LDS = (size_t)KEPT_LDS * (16 + 16 + 4 + 4) + (size_t)16 * 64 * (16 + 4);

struct StitchKept {  // the per-kept arrays of the segment at seg0: rank < KEPT_LDS in LDS, later ranks in the workspace at seg0 + rank
  float4 *s_box, *s_u, *g_box, *g_u;
  unsigned *s_meta, *s_row, *g_meta, *g_row;
  size_t seg0;
  __device__ __forceinline__ float4& box(int r) const { return r < KEPT_LDS ? s_box[r] : g_box[seg0 + r]; }
  __device__ __forceinline__ float4& u(int r) const { return r < KEPT_LDS ? s_u[r] : g_u[seg0 + r]; }
  __device__ __forceinline__ unsigned& meta(int r) const { return r < KEPT_LDS ? s_meta[r] : g_meta[seg0 + r]; }
  __device__ __forceinline__ unsigned& row(int r) const { return r < KEPT_LDS ? s_row[r] : g_row[seg0 + r]; }
};

// wave 0: every lane with `on` adds one to the count of kept box r and, with `hull`, its box b to that box's U.  Lanes that name the same
// r are folded in the wave first (min / max, a popcount), so one lane updates r once
__device__ __forceinline__ void stitch_absorb(const StitchKept& k, int lane, bool on, int r, bool hull, float4 b) {
  const float inf = __builtin_inff();
  unsigned long long pend = __ballot(on);
  while (pend) {
    const int lead = __ffsll((long long)pend) - 1;
    const int r0 = __shfl(r, lead);
    const bool mine = on && r == r0;
    const unsigned long long m = __ballot(mine);
    pend &= ~m;
    if (hull) {
      float x1 = mine ? b.x : inf, y1 = mine ? b.y : inf, x2 = mine ? b.z : -inf, y2 = mine ? b.w : -inf;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        x1 = fminf(x1, __shfl_xor(x1, o)); y1 = fminf(y1, __shfl_xor(y1, o));
        x2 = fmaxf(x2, __shfl_xor(x2, o)); y2 = fmaxf(y2, __shfl_xor(y2, o));
      }
      if (lane == lead) {
        const float4 u = k.u(r0);
        k.u(r0) = make_float4(fminf(u.x, x1), fminf(u.y, y1), fmaxf(u.z, x2), fmaxf(u.w, y2));
      }
    }
    if (lane == lead) k.meta(r0) += (unsigned)__popcll(m);
    __threadfence_block();  // (a spilled box may be updated again, by another lane)
  }
}

__global__ __launch_bounds__(1024) void stitch_walk_kernel(const ulonglong2* __restrict__ keys, unsigned P, const MergeView* __restrict__ views,
                                                           const StitchView* __restrict__ sviews, int max_in, const float* __restrict__ boxes,
                                                           float thr, float sthr, float border, float4* kbox, float4* ubox, unsigned* kmeta,
                                                           unsigned* krow, float4* __restrict__ out_u, int* __restrict__ out_cnt) {
  extern __shared__ __attribute__((aligned(16))) unsigned char stitch_lds[];
  float4* s_kept = reinterpret_cast<float4*>(stitch_lds);
  float4* s_u = s_kept + KEPT_LDS;
  float4* s_stage = s_u + KEPT_LDS;  // [16][64], per wave: the group of spilled kept boxes (4b: of their U) it is comparing against
  unsigned* s_meta = reinterpret_cast<unsigned*>(s_stage + 16 * 64);
  unsigned* s_row = s_meta + KEPT_LDS;
  unsigned* s_stagem = s_row + KEPT_LDS;  // [16][64]
  __shared__ int s_best[16][64];
  __shared__ unsigned s_d[64][2];
  __shared__ float4 s_box4[64], s_u4[64];
  __shared__ unsigned long long s_starts, s_valid, s_cutm;
  __shared__ int s_kept_total, s_last, s_any_cut;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const unsigned p0 = blockIdx.x * 64u;
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned long long starts = segment_starts(keys, p0, &s_starts);
  while (starts) {
    const unsigned seg0 = p0 + (unsigned)(__ffsll((long long)starts) - 1);
    starts &= starts - 1;
    const unsigned long long seg_hi = keys[seg0].x;
    const StitchKept kl = {s_kept, s_u, kbox, ubox, s_meta, s_row, kmeta, krow, (size_t)seg0};
    int kept_total = 0;  // wave 0 keeps the running state; mirrored in LDS for the other waves
    bool any_cut = false;
    if (t == 0) s_kept_total = 0;
    // rule 4a
    for (unsigned c = 0;; ++c) {
      const unsigned long long pos = (unsigned long long)seg0 + 64ull * c + (unsigned)lane;
      unsigned g = 0u;
      if (wave == 0) {
        unsigned long long lo;
        float4 bx;
        bool cut = false;
        if (segment_chunk_load(keys, P, pos, seg_hi, boxes, views, max_in, lane, s_box4, s_d, &s_valid, &lo, &bx)) {
          g = (unsigned)(lo & 0xffffffffull);
          const unsigned v = g / (unsigned)max_in;
          cut = stitch_cut(bx, views[v], sviews[v], border);
        }
        const unsigned long long cm = __ballot(cut);
        if (lane == 0) s_cutm = cm;
      }
      __syncthreads();
      const int ktot = s_kept_total;
      const unsigned long long vmask = s_valid, cutm = s_cutm;
      const float4 mb = s_box4[lane];
      const bool mcut = (cutm >> lane) & 1ull;
      int best = NO_KEEPER;  // the lowest rank this wave's groups hold of a kept box that matches the lane's (ranks ascend along the loop)
      walk_kept_groups<false, true>(ktot, lane, wave, mb, s_kept, kbox + seg0, s_stage, s_meta, kmeta + seg0, s_stagem,
                                    [&](int r, float4 kb, unsigned meta) {
                                      const bool pair_cut = mcut || (meta & META_CUT);
                                      if (best == NO_KEEPER && stitch_match(kb, mb, pair_cut, thr, sthr)) best = r;
                                    });
      {
        const float4 ib = s_box4[t >> 4];
        const bool icut = (cutm >> (t >> 4)) & 1ull;
        walk_fill_matrix(s_d, t, [&](int, int j) { return stitch_match(ib, s_box4[j], icut || ((cutm >> j) & 1ull), thr, sthr); });
      }
      s_best[wave][lane] = best;
      __syncthreads();
      if (wave == 0) {
        int ext = NO_KEEPER;  // the keeper among the boxes kept in earlier chunks: they all rank below this chunk's
#pragma unroll
        for (int w = 0; w < 16; ++w) ext = min(ext, s_best[w][lane]);
        const unsigned long long cur = ~vmask | __ballot(ext != NO_KEEPER);  // the lanes past the segment's end are never kept
        int ink;  // the first box kept in this chunk that matches the lane's
        const unsigned long long keptmask = walk_resolve<true>(cur, s_d, lane, &ink);
        const bool valid = (vmask >> lane) & 1ull, is_kept = (keptmask >> lane) & 1ull;
        const int rank = kept_total + __popcll(keptmask & below);
        if (is_kept) {
          kl.box(rank) = mb;
          kl.u(rank) = mb;
          kl.meta(rank) = mcut ? META_CUT : 0u;
          kl.row(rank) = g;
        }
        __threadfence_block();
        const bool absorbed = valid && !is_kept;
        int keeper = 0;
        bool kcut = false;
        if (absorbed) {
          if (ext != NO_KEEPER) {
            keeper = ext;
            kcut = kl.meta(ext) & META_CUT;
          } else {  // (ink >= 0: an absorbed row without a keeper before the chunk has one inside)
            keeper = kept_total + __popcll(keptmask & ((1ull << ink) - 1ull));
            kcut = (cutm >> ink) & 1ull;
          }
        }
        stitch_absorb(kl, lane, absorbed && (mcut || kcut), keeper, true, mb);  // an uncut pair only suppresses
        any_cut = any_cut || (keptmask & cutm) != 0ull;
        kept_total += __popcll(keptmask);
        if (lane == 0) { s_kept_total = kept_total; s_last = vmask != ~0ull ? 1 : 0; s_any_cut = any_cut ? 1 : 0; }
      }
      __syncthreads();
      if (s_last) break;
    }
    // rule 4b: only a cut kept box can be dropped
    const int ktotal = s_kept_total;
    if (s_any_cut) {
      for (int k0 = 0; k0 < ktotal; k0 += 64) {
        if (wave == 0) {
          const bool valid = k0 + lane < ktotal;
          const unsigned meta = valid ? kl.meta(k0 + lane) : 0u;
          s_box4[lane] = valid ? kl.box(k0 + lane) : make_float4(0.f, 0.f, 0.f, 0.f);
          s_u4[lane] = valid ? kl.u(k0 + lane) : make_float4(0.f, 0.f, 0.f, 0.f);
          s_d[lane][0] = 0u; s_d[lane][1] = 0u;
          const unsigned long long cm = __ballot((meta & META_CUT) != 0u);
          if (lane == 0) s_cutm = cm;
        }
        __syncthreads();
        const unsigned long long cutm = s_cutm;
        if (cutm == 0ull) {  // (uniform) nothing to drop here, and the boxes stay what they are for the later chunks
          __syncthreads();
          continue;
        }
        const float4 mb = s_box4[lane];
        const bool mcut = (cutm >> lane) & 1ull;
        int best = NO_KEEPER;
        // against the frozen U of the earlier chunks' ranks (k0 is a multiple of 64: full groups)
        walk_kept_groups<false, true>(k0, lane, wave, mb, s_u, ubox + seg0, s_stage, s_meta, kmeta + seg0, s_stagem,
                                      [&](int r, float4 ub, unsigned meta) {
                                        if (best == NO_KEEPER && mcut && !(meta & META_DROPPED) && stitch_covered(ub, mb, sthr)) best = r;
                                      });
        {
          const float4 iu = s_u4[t >> 4];
          walk_fill_matrix(s_d, t, [&](int, int j) { return ((cutm >> j) & 1ull) && stitch_covered(iu, s_box4[j], sthr); });
        }
        s_best[wave][lane] = best;
        __syncthreads();
        if (wave == 0) {
          int ext = NO_KEEPER;
#pragma unroll
          for (int w = 0; w < 16; ++w) ext = min(ext, s_best[w][lane]);
          int ink;  // the first survivor of this chunk whose U holds the lane's box
          const unsigned long long alive = walk_resolve<true>(__ballot(ext != NO_KEEPER), s_d, lane, &ink);
          const bool dropped = !((alive >> lane) & 1ull);  // (a lane past the end has no cut bit: never dropped)
          if (dropped) kl.meta(k0 + lane) |= META_DROPPED;
          __threadfence_block();
          stitch_absorb(kl, lane, dropped, ext != NO_KEEPER ? ext : k0 + ink, false, mb);
        }
        __syncthreads();
      }
    }
    for (int r = t; r < ktotal; r += 1024) {
      const unsigned meta = kl.meta(r);
      if (meta & META_DROPPED) continue;
      const unsigned g = kl.row(r);
      out_u[g] = kl.u(r);
      out_cnt[g] = 1 + (int)(meta & META_COUNT);
    }
    __syncthreads();
  }
}

// the head both launches share: status and bounds cleared (and `clear`, when given), the keys, the first sort when asked for
int large_head(const MergeLargeLayout& L, char* ws, int n_src, const MergeView* views, int max_in, const float* scores, const int* classes,
               const int* counts, int* status, void* clear, size_t clear_bytes, bool sort, hipStream_t s) {
  ulonglong2* keys = reinterpret_cast<ulonglong2*>(ws + L.keys_off);
  const unsigned P = (unsigned)L.P;
  if (hipMemsetAsync(status, 0, sizeof(int), s) != hipSuccess) return -8;
  if (hipMemsetAsync(ws + L.bounds_off, 0, (size_t)2 * n_src * sizeof(unsigned), s) != hipSuccess) return -8;
  if (clear && hipMemsetAsync(clear, 0, clear_bytes, s) != hipSuccess) return -8;
  hipLaunchKernelGGL(merge_large_keys_kernel, dim3((P + 255) / 256), dim3(256), 0, s, keys, P, (unsigned)L.rows, max_in, views, scores, classes, counts);
  if (sort) sort_keys(keys, P, s);
  return 0;
}

// the tail both launches share: the second keys (kept / nms_on of the large merge, or the stitching merge's cnt), their sort, the bounds
// and the emit (ubox and out_stitched: the stitching merge's)
template <bool STITCH>
int large_tail(const MergeLargeLayout& L, char* ws, int n_src, const MergeView* views, int max_in, const float* boxes, const float* scores,
               const int* classes, const unsigned char* kept, int nms_on, const float4* ubox, const int* cnt, int K, int max_out, float* out_boxes,
               float* out_scores, int* out_classes, int* out_view, int* out_row, int* out_stitched, int* out_counts, int* status, hipStream_t s) {
  ulonglong2* keys = reinterpret_cast<ulonglong2*>(ws + L.keys_off);
  unsigned* bounds = reinterpret_cast<unsigned*>(ws + L.bounds_off);
  const unsigned P = (unsigned)L.P, flat = (P + 255) / 256;
  hipLaunchKernelGGL(merge_large_rekey_kernel<STITCH>, dim3(flat), dim3(256), 0, s, keys, P, kept, nms_on, cnt);
  sort_keys(keys, P, s);
  hipLaunchKernelGGL(merge_large_bounds_kernel, dim3(flat), dim3(256), 0, s, keys, P, bounds);
  const int bps = max_out / 256 + 1;  // max_out + 1 threads per source
  if ((long long)bps * n_src > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(merge_large_emit_kernel<STITCH>, dim3((unsigned)bps * n_src), dim3(256), 0, s, keys, bounds, views, max_in, boxes, ubox, cnt,
                     scores, classes, K, max_out, bps, out_boxes, out_scores, out_classes, out_view, out_row, out_stitched, out_counts, status);
  return (int)hipGetLastError();
}

}  // namespace

int launch_stitch_views(int n_src, int n_views, const MergeView* views, const StitchView* sviews, int max_in, const float* boxes,
                        const float* scores, const int* classes, const int* counts, float nms_thresh, float stitch_thr, float border_px, int K,
                        int max_out, float* out_boxes, float* out_scores, int* out_classes, int* out_view, int* out_row, int* out_stitched,
                        int* out_counts, int* status, void* workspace, hipStream_t s) {
  const MergeLargeLayout L = stitch_layout(n_src, n_views, max_in);
  if (L.bytes < 0 || max_out <= 0 || !workspace) return (int)hipErrorInvalidValue;
  static PerDeviceOnce once;
  if (!once.run(current_device(), [] {
        return hipFuncSetAttribute((const void*)stitch_walk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)STITCH_LDS) == hipSuccess;
      }))
    return -7;
  char* ws = static_cast<char*>(workspace);
  ulonglong2* keys = reinterpret_cast<ulonglong2*>(ws + L.keys_off);
  float4* out_u = reinterpret_cast<float4*>(ws + L.outu_off);
  int* out_cnt = reinterpret_cast<int*>(ws + L.outc_off);
  // (the first sort also with NMS off: a cut pair matches whatever NMS_TH is)
  if (const int r = large_head(L, ws, n_src, views, max_in, scores, classes, counts, status, out_cnt, (size_t)L.rows * sizeof(int), true, s)) return r;
  hipLaunchKernelGGL(stitch_walk_kernel, dim3((unsigned)L.P / 64), dim3(1024), STITCH_LDS, s, keys, (unsigned)L.P, views, sviews, max_in, boxes,
                     nms_thresh, stitch_thr, border_px, reinterpret_cast<float4*>(ws + L.kbox_off), reinterpret_cast<float4*>(ws + L.ubox_off),
                     reinterpret_cast<unsigned*>(ws + L.meta_off), reinterpret_cast<unsigned*>(ws + L.row_off), out_u, out_cnt);
  return large_tail<true>(L, ws, n_src, views, max_in, boxes, scores, classes, nullptr, 0, out_u, out_cnt, K, max_out, out_boxes, out_scores,
                          out_classes, out_view, out_row, out_stitched, out_counts, status, s);
}

int launch_merge_views_large(int n_src, int n_views, const MergeView* views, int max_in, const float* boxes, const float* scores,
                             const int* classes, const int* counts, float nms_thresh, int K, int max_out, float* out_boxes, float* out_scores,
                             int* out_classes, int* out_view, int* out_row, int* out_counts, int* status, void* workspace, hipStream_t s) {
  const MergeLargeLayout L = merge_large_layout(n_src, n_views, max_in);
  if (L.bytes < 0 || max_out <= 0 || !workspace) return (int)hipErrorInvalidValue;
  char* ws = static_cast<char*>(workspace);
  ulonglong2* keys = reinterpret_cast<ulonglong2*>(ws + L.keys_off);
  unsigned char* kept = reinterpret_cast<unsigned char*>(ws + L.kept_off);
  const int nms_on = nms_thresh > 0.f ? 1 : 0;
  if (const int r = large_head(L, ws, n_src, views, max_in, scores, classes, counts, status, nullptr, 0, nms_on != 0, s)) return r;
  if (nms_on) {
    if (hipMemsetAsync(kept, 0, (size_t)L.rows, s) != hipSuccess) return -8;
    hipLaunchKernelGGL(merge_large_nms_kernel, dim3((unsigned)L.P / 64), dim3(1024), 0, s, keys, (unsigned)L.P, views, max_in, boxes, nms_thresh, K,
                       reinterpret_cast<float4*>(ws + L.kbox_off), kept);
  }
  return large_tail<false>(L, ws, n_src, views, max_in, boxes, scores, classes, kept, nms_on, nullptr, nullptr, K, max_out, out_boxes, out_scores,
                           out_classes, out_view, out_row, nullptr, out_counts, status, s);
}

}  // namespace sylph
