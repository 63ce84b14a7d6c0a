// COCO bbox evaluation on the device (pycocotools' COCOeval.evaluateImg / accumulate, useCats = 1): gfx950.
// All arithmetic that reaches a result is float64 in the order of tests/cocoeval_ref.py; this file is built without FMA contraction.
//
// coco_match_kernel: one wave per (image, category) pair.  The pair's detections arrive ordered by score (stable) and are cut to max_det;
//   1  detection boxes XYXY fp32 -> XYWH float64 in LDS; per ground-truth box a 64-byte state row: bytes 0..39 "matched at (area, threshold)
//      lane", byte 63 = crowd << 4 | ignored-in-area-range bits
//   2  the D x G IoU tile, float64, into LDS (pairs of more than tile_g boxes: no tile, the IoU is recomputed at every visit, and the
//      state rows live in the caller's scratch)
//   3  the greedy walk: lane a * T + t owns (area range a, threshold t) and walks the detections in order; per detection it visits the
//      non-ignored boxes in file order, then -- only while unmatched -- the ignored ones.  All lanes read the same tile entry (LDS
//      broadcast); the walk is sequential in detections by definition, the 40 combinations are the parallel axis
//   4  per detection two ballots give the 40-bit matched / ignored masks; lanes t == 0 add the pair's non-ignored count to npig[k][a]
// coco_accumulate_kernel: one block per (category, area range, maxDet) cell, all thresholds at once, over the category's segment of the
//   rows ordered by (category, score): a counting pass for the totals, then the chunks from the last to the first -- block scan of the
//   chunk's tp / fp counts (carry = totals minus what the later chunks held), precision per row, suffix maximum across the chunk with
//   the later chunks' maximum as carry, and at every row where the recall steps the recall thresholds it is the first to reach.
#include "common.h"
#include "kernels.h"
#include "eval_iou.h"

namespace sylph {

typedef unsigned long long u64;

// dynamic LDS: detection boxes [max_det][4] f64 | IoU tile [max_det][tile_g] f64 | state rows [tile_g][64] bytes
__global__ __launch_bounds__(64) void coco_match_kernel(const float* __restrict__ det, const int* __restrict__ det_off,
                                                        const double* __restrict__ gt_box, const double* __restrict__ gt_area,
                                                        const int* __restrict__ gt_crowd, const int* __restrict__ gt_off, int K,
                                                        const double* __restrict__ iou_thr, int T, const double* __restrict__ area_rng, int A,
                                                        int max_det, int tile_g, unsigned char* gt_scratch, u64* matched, u64* ignored,
                                                        int* npig) {
  extern __shared__ double coco_lds[];
  const int p = blockIdx.x, lane = threadIdx.x;
  const int d0 = det_off[p], nd = det_off[p + 1] - d0;
  const int g0 = gt_off[p], G = gt_off[p + 1] - g0;
  if (nd == 0 && G == 0) return;  // the pair does not exist
  const int D = nd < max_det ? nd : max_det;
  double* dbox = coco_lds;
  double* tile = dbox + (size_t)max_det * 4;
  const bool big = G > tile_g;
  unsigned char* gs = big ? gt_scratch + (size_t)g0 * 64 : reinterpret_cast<unsigned char*>(tile + (size_t)max_det * tile_g);

  for (int i = lane; i < D; i += 64) {
    const float* r = det + (size_t)(d0 + i) * 8;
    const double x0 = (double)r[1], y0 = (double)r[2], x1 = (double)r[3], y1 = (double)r[4];
    dbox[i * 4 + 0] = x0;
    dbox[i * 4 + 1] = y0;
    dbox[i * 4 + 2] = x1 - x0;
    dbox[i * 4 + 3] = y1 - y0;
  }
  for (int g = lane; g < G; g += 64) {
    const double ar = gt_area[g0 + g];
    const int crowd = gt_crowd[g0 + g] != 0;
    unsigned f = crowd ? 0x10u : 0u;
    for (int a = 0; a < A; ++a)
      if (crowd || ar < area_rng[2 * a] || ar > area_rng[2 * a + 1]) f |= 1u << a;
    u64* row = reinterpret_cast<u64*>(gs + (size_t)g * 64);
    for (int q = 0; q < 7; ++q) row[q] = 0ull;
    row[7] = (u64)f << 56;  // byte 63
  }
  __syncthreads();
  if (!big) {
    const int cells = D * G;
    for (int idx = lane; idx < cells; idx += 64) {
      const int d = idx / G, g = idx - d * G;
      tile[idx] = coco_iou(dbox[d * 4], dbox[d * 4 + 1], dbox[d * 4 + 2], dbox[d * 4 + 3], gt_box + (size_t)(g0 + g) * 4, gt_crowd[g0 + g] != 0);
    }
  }
  __syncthreads();

  const bool act = lane < A * T;
  const int a = act ? lane / T : 0, t = act ? lane - a * T : 0;
  const double thr0 = fmin(iou_thr[t], 1.0 - 1e-10);
  const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
  if (act && t == 0) {
    int cnt = 0;
    for (int g = 0; g < G; ++g) cnt += ((gs[(size_t)g * 64 + 63] >> a) & 1) ? 0 : 1;
    if (cnt) atomicAdd(&npig[(p % K) * A + a], cnt);
  }
  for (int d = 0; d < D; ++d) {
    int m = -1;
    bool dig = false;
    if (act) {
      const double dx = dbox[d * 4], dy = dbox[d * 4 + 1], dw = dbox[d * 4 + 2], dh = dbox[d * 4 + 3];
      double best = thr0;
      for (int pass = 0; pass < 2; ++pass) {  // non-ignored boxes first; the ignored ones only while nothing is matched
        if (pass == 1 && m >= 0) break;
        for (int g = 0; g < G; ++g) {
          const unsigned f = gs[(size_t)g * 64 + 63];
          if ((int)((f >> a) & 1u) != pass) continue;
          const int crowd = (f >> 4) & 1u;
          if (gs[(size_t)g * 64 + lane] && !crowd) continue;
          const double iou = big ? coco_iou(dx, dy, dw, dh, gt_box + (size_t)(g0 + g) * 4, crowd) : tile[(size_t)d * G + g];
          if (iou < best) continue;
          best = iou;  // an equal IoU replaces: the last of equal candidates wins
          m = g;
        }
      }
      if (m >= 0) {
        gs[(size_t)m * 64 + lane] = 1;
        dig = (gs[(size_t)m * 64 + 63] >> a) & 1u;
      } else {
        const double da = dw * dh;
        dig = da < lo || da > hi;
      }
    }
    const u64 mm = __ballot(act && m >= 0), ii = __ballot(act && dig);
    if (lane == 0) {
      matched[d0 + d] = mm;
      ignored[d0 + d] = ii;
    }
  }
}

int launch_coco_match(int n_pairs, int K, const float* det, const int* det_off, const double* gt_box, const double* gt_area, const int* gt_crowd,
                      const int* gt_off, int max_gt, const double* iou_thr, int T, const double* area_rng, int A, int max_det,
                      unsigned char* gt_scratch, u64* matched, u64* ignored, int* npig, hipStream_t s) {
  if (n_pairs <= 0 || K <= 0 || T <= 0 || A <= 0 || A > 4 || A * T > COCO_MATCH_LANES || max_det <= 0 || max_det > COCO_MATCH_MAX_DETS || max_gt < 0)
    return (int)hipErrorInvalidValue;
  const size_t dbox = (size_t)max_det * 32, per_g = (size_t)max_det * 8 + 64;
  size_t tile_g = (size_t)coco_match_tile_gt(max_det);
  if ((size_t)max_gt > tile_g && !gt_scratch) return (int)hipErrorInvalidValue;  // a pair past the tile keeps its flags in the scratch
  if (tile_g > (size_t)max_gt) tile_g = max_gt;
  const size_t lds = dbox + tile_g * per_g;
  static PerDeviceOnce once;
  if (!once.run(current_device(), [] {
        return hipFuncSetAttribute((const void*)coco_match_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, COCO_MATCH_LDS_BYTES) == hipSuccess;
      }))
    return -7;
  if (hipMemsetAsync(npig, 0, (size_t)K * A * sizeof(int), s) != hipSuccess) return -8;
  hipLaunchKernelGGL(coco_match_kernel, dim3(n_pairs), dim3(64), lds, s, det, det_off, gt_box, gt_area, gt_crowd, gt_off, K, iou_thr, T, area_rng, A,
                     max_det, (int)tile_g, gt_scratch, matched, ignored, npig);
  return (int)hipGetLastError();
}

// ---- accumulate -------------------------------------------------------------------------------------------------------------------
constexpr int ACC_THREADS = 256, ACC_ROWS = COCO_ACC_CHUNK / ACC_THREADS, ACC_WAVES = ACC_THREADS / 64;
constexpr int ACC_T = COCO_MAX_THRESHOLDS, ACC_R = COCO_MAX_REC_THRESHOLDS;
static_assert(ACC_ROWS * ACC_THREADS == COCO_ACC_CHUNK && COCO_ACC_CHUNK < 65536, "a chunk's tp / fp counts share a 32-bit word");

// how many of the ascending thr[0 .. R) are <= x, for x in [0, 1]: a guess that is right for evenly spaced thresholds, then single steps
// (correct for any ascending table; the steps only cost time when the guess is off)
__device__ __forceinline__ int coco_count_le(const double* thr, int R, double x) {
  int i = (int)(x * (double)(R - 1)) + 1;
  i = i < 0 ? 0 : (i > R ? R : i);
  while (i < R && thr[i] <= x) ++i;
  while (i > 0 && thr[i - 1] > x) --i;
  return i;
}

__global__ __launch_bounds__(ACC_THREADS) void coco_accumulate_kernel(const float* __restrict__ score, const int* __restrict__ rank,
                                                                      const u64* __restrict__ matched, const u64* __restrict__ ignored,
                                                                      const int* __restrict__ cat_off, const int* __restrict__ npig,
                                                                      const int* __restrict__ max_dets, const double* __restrict__ rec_thr, int T,
                                                                      int R, int K, int A, int M, double* precision, double* recall,
                                                                      double* scores) {
  __shared__ double s_prec[ACC_T][ACC_R], s_score[ACC_T][ACC_R], s_thr[ACC_R], s_wmax[ACC_WAVES][ACC_T];
  __shared__ int s_tot[2 * ACC_T + 1];
  __shared__ unsigned s_wsum[ACC_WAVES][ACC_T + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cell = blockIdx.x, m = cell % M, a = (cell / M) % A, k = cell / (M * A);
  const int np = npig[k * A + a], md = max_dets[m];
  const int r0 = cat_off[k], L = cat_off[k + 1] - r0;
  const unsigned tmask = (1u << T) - 1u;
  const int shift = a * T;
  const double fill = np == 0 ? -1.0 : 0.0;
  for (int i = tid; i < ACC_T * ACC_R; i += ACC_THREADS) {
    (&s_prec[0][0])[i] = fill;
    (&s_score[0][0])[i] = fill;
  }
  for (int i = tid; i < R; i += ACC_THREADS) s_thr[i] = rec_thr[i];
  if (tid < 2 * ACC_T + 1) s_tot[tid] = 0;
  __syncthreads();

  int tot_tp[ACC_T], tot_fp[ACC_T], ntot = 0;
  if (np != 0) {
    // totals
    int ctp[ACC_T], cfp[ACC_T], cn = 0;
#pragma unroll
    for (int t = 0; t < ACC_T; ++t) ctp[t] = cfp[t] = 0;
    for (int i0 = tid; i0 < L; i0 += ACC_THREADS * ACC_ROWS) {
      int rk[ACC_ROWS];
      u64 mw[ACC_ROWS], iw[ACC_ROWS];
#pragma unroll
      for (int j = 0; j < ACC_ROWS; ++j) {  // independent loads: one round trip for the rows of an iteration
        const int i = i0 + j * ACC_THREADS;
        const bool in = i < L;
        rk[j] = in ? rank[r0 + i] : md;
        mw[j] = in ? matched[r0 + i] : 0ull;
        iw[j] = in ? ignored[r0 + i] : 0ull;
      }
#pragma unroll
      for (int j = 0; j < ACC_ROWS; ++j) {
        if (rk[j] >= md) continue;
        const unsigned mt = (unsigned)(mw[j] >> shift) & tmask, ig = (unsigned)(iw[j] >> shift) & tmask;
        const unsigned tpb = mt & ~ig, fpb = ~mt & ~ig & tmask;
        ++cn;
#pragma unroll
        for (int t = 0; t < ACC_T; ++t) {
          ctp[t] += (tpb >> t) & 1u;
          cfp[t] += (fpb >> t) & 1u;
        }
      }
    }
#pragma unroll
    for (int t = 0; t < ACC_T; ++t) {
      if (ctp[t]) atomicAdd(&s_tot[t], ctp[t]);
      if (cfp[t]) atomicAdd(&s_tot[ACC_T + t], cfp[t]);
    }
    if (cn) atomicAdd(&s_tot[2 * ACC_T], cn);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < ACC_T; ++t) {
      tot_tp[t] = s_tot[t];
      tot_fp[t] = s_tot[ACC_T + t];
    }
    ntot = s_tot[2 * ACC_T];

    // chunks, last to first
    const double dnp = (double)np, eps = 2.220446049250313e-16;  // np.spacing(1)
    int end_tp[ACC_T], end_fp[ACC_T], end_n = ntot;  // counts up to the end of the current chunk
    double cmax[ACC_T];                              // precision maximum of the later chunks
#pragma unroll
    for (int t = 0; t < ACC_T; ++t) {
      end_tp[t] = tot_tp[t];
      end_fp[t] = tot_fp[t];
      cmax[t] = -1.0;
    }
    const int nchunks = (L + COCO_ACC_CHUNK - 1) / COCO_ACC_CHUNK;
    for (int c = nchunks - 1; c >= 0; --c) {
      const int base = c * COCO_ACC_CHUNK + tid * ACC_ROWS;
      unsigned tpb[ACC_ROWS], fpb[ACC_ROWS];
      bool keep[ACC_ROWS];
      float sc[ACC_ROWS];
      unsigned v[ACC_T + 1];
#pragma unroll
      for (int t = 0; t <= ACC_T; ++t) v[t] = 0u;
      int rk[ACC_ROWS];
      u64 mw[ACC_ROWS], iw[ACC_ROWS];
#pragma unroll
      for (int j = 0; j < ACC_ROWS; ++j) {  // independent loads: one round trip per chunk
        const int i = base + j;
        const bool in = i < L;
        rk[j] = in ? rank[r0 + i] : md;
        mw[j] = in ? matched[r0 + i] : 0ull;
        iw[j] = in ? ignored[r0 + i] : 0ull;
        sc[j] = in ? score[r0 + i] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < ACC_ROWS; ++j) {
        keep[j] = rk[j] < md;
        tpb[j] = fpb[j] = 0u;
        if (keep[j]) {
          const unsigned mt = (unsigned)(mw[j] >> shift) & tmask, ig = (unsigned)(iw[j] >> shift) & tmask;
          tpb[j] = mt & ~ig;
          fpb[j] = ~mt & ~ig & tmask;
          ++v[ACC_T];
#pragma unroll
          for (int t = 0; t < ACC_T; ++t) v[t] += ((tpb[j] >> t) & 1u) | (((fpb[j] >> t) & 1u) << 16);
        }
      }
      // exclusive prefix of v over the block (tp in the low half, fp in the high half of a word)
      unsigned inc[ACC_T + 1];
#pragma unroll
      for (int t = 0; t <= ACC_T; ++t) inc[t] = v[t];
      for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
        for (int t = 0; t <= ACC_T; ++t) {
          const unsigned x = __shfl_up(inc[t], off);
          if (lane >= off) inc[t] += x;
        }
      }
      // suffix maximum needs the rows' precisions first; the wave sums go to LDS now
      if (lane == 63) {
#pragma unroll
        for (int t = 0; t <= ACC_T; ++t) s_wsum[wave][t] = inc[t];
      }
      __syncthreads();
      unsigned ex[ACC_T + 1], ctot[ACC_T + 1];
#pragma unroll
      for (int t = 0; t <= ACC_T; ++t) {
        unsigned before = 0u, all = 0u;
        for (int w = 0; w < ACC_WAVES; ++w) {
          const unsigned x = s_wsum[w][t];
          if (w < wave) before += x;
          all += x;
        }
        ex[t] = before + inc[t] - v[t];
        ctot[t] = all;
      }
      // counts before this thread's first row
      int tp[ACC_T], fp[ACC_T];
#pragma unroll
      for (int t = 0; t < ACC_T; ++t) {
        tp[t] = end_tp[t] - (int)(ctot[t] & 0xffffu) + (int)(ex[t] & 0xffffu);
        fp[t] = end_fp[t] - (int)(ctot[t] >> 16) + (int)(ex[t] >> 16);
      }
      const int fidx0 = end_n - (int)ctot[ACC_T] + (int)ex[ACC_T];  // index of this thread's first kept row among the kept rows
      double pr[ACC_ROWS][ACC_T], lmax[ACC_T];
#pragma unroll
      for (int t = 0; t < ACC_T; ++t) lmax[t] = -1.0;
#pragma unroll
      for (int j = 0; j < ACC_ROWS; ++j) {
#pragma unroll
        for (int t = 0; t < ACC_T; ++t) {
          pr[j][t] = -1.0;
          if (keep[j]) {
            tp[t] += (tpb[j] >> t) & 1u;
            fp[t] += (fpb[j] >> t) & 1u;
            pr[j][t] = (double)tp[t] / ((double)fp[t] + (double)tp[t] + eps);
            lmax[t] = fmax(lmax[t], pr[j][t]);
          }
        }
      }
      // maximum over the rows behind this thread: later lanes, later waves, later chunks
      double sfx[ACC_T];
#pragma unroll
      for (int t = 0; t < ACC_T; ++t) sfx[t] = lmax[t];
      for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
        for (int t = 0; t < ACC_T; ++t) {
          const double x = __shfl_down(sfx[t], off);
          if (lane + off < 64) sfx[t] = fmax(sfx[t], x);
        }
      }
      if (lane == 0) {
#pragma unroll
        for (int t = 0; t < ACC_T; ++t) s_wmax[wave][t] = sfx[t];
      }
      __syncthreads();
      double run[ACC_T];
#pragma unroll
      for (int t = 0; t < ACC_T; ++t) {
        const double nxt = __shfl_down(sfx[t], 1);
        double r = lane < 63 ? nxt : -1.0;
        double all = cmax[t];
        for (int w = 0; w < ACC_WAVES; ++w) {
          const double x = s_wmax[w][t];
          if (w > wave) r = fmax(r, x);
          all = fmax(all, x);
        }
        run[t] = fmax(r, cmax[t]);
        cmax[t] = all;
      }
      // rows of this thread from the last to the first: tp[] holds the count after the last one
      int nk = 0;
#pragma unroll
      for (int j = 0; j < ACC_ROWS; ++j) nk += keep[j] ? 1 : 0;
      int fidx = fidx0 + nk;
#pragma unroll
      for (int j = ACC_ROWS - 1; j >= 0; --j) {
        if (!keep[j]) continue;
        --fidx;
#pragma unroll
        for (int t = 0; t < ACC_T; ++t) {
          if (t >= T) continue;
          run[t] = fmax(run[t], pr[j][t]);
          const int step = (tpb[j] >> t) & 1u;
          if (step || fidx == 0) {
            // the recall thresholds this row is the first to reach: rc[fidx - 1] < thr <= rc[fidx]
            const int hi_r = coco_count_le(s_thr, R, (double)tp[t] / dnp);
            const double rc_prev = fidx == 0 ? -__builtin_huge_val() : (double)(tp[t] - step) / dnp;
            for (int r = hi_r - 1; r >= 0 && s_thr[r] > rc_prev; --r) {
              s_prec[t][r] = run[t];
              s_score[t][r] = (double)sc[j];
            }
          }
          tp[t] -= step;
        }
      }
#pragma unroll
      for (int t = 0; t < ACC_T; ++t) {
        end_tp[t] -= (int)(ctot[t] & 0xffffu);
        end_fp[t] -= (int)(ctot[t] >> 16);
      }
      end_n -= (int)ctot[ACC_T];
      __syncthreads();  // s_wsum / s_wmax are rewritten by the next chunk
    }
  }
  __syncthreads();
  for (int i = tid; i < T * R; i += ACC_THREADS) {
    const int t = i / R, r = i - t * R;
    const size_t o = ((((size_t)t * R + r) * K + k) * A + a) * M + m;
    precision[o] = s_prec[t][r];
    scores[o] = s_score[t][r];
  }
  if (tid < T) {
    double rc = -1.0;
    if (np != 0) {
      rc = 0.0;
#pragma unroll
      for (int t = 0; t < ACC_T; ++t)
        if (t == tid && ntot > 0) rc = (double)tot_tp[t] / (double)np;
    }
    recall[(((size_t)tid * K + k) * A + a) * M + m] = rc;
  }
}

int launch_coco_accumulate(const float* score, const int* rank, const u64* matched, const u64* ignored, int K, const int* cat_off, const int* npig,
                           int T, int R, const double* rec_thr, int A, int M, const int* max_dets, double* precision, double* recall,
                           double* scores, hipStream_t s) {
  if (K <= 0 || T <= 0 || T > COCO_MAX_THRESHOLDS || R <= 0 || R > COCO_MAX_REC_THRESHOLDS || A <= 0 || A > 4 || A * T > COCO_MATCH_LANES || M <= 0)
    return (int)hipErrorInvalidValue;
  if ((long)K * A * M >= (1L << 31)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(coco_accumulate_kernel, dim3(K * A * M), dim3(ACC_THREADS), 0, s, score, rank, matched, ignored, cat_off, npig, max_dets, rec_thr,
                     T, R, K, A, M, precision, recall, scores);
  return (int)hipGetLastError();
}

}  // namespace sylph
