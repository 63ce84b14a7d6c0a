// Host side of libsylph_hip.so, unit "eval": COCO bbox matching and accumulation on detection rows (sylph_coco_match, sylph_coco_accumulate)
// and LVIS matching over a compacted pair list (sylph_lvis_match).
// No torch types, no CPU compute fallback: the stages are HIP kernels of coco_eval.hip and lvis_eval.hip.
#include "api_internal.h"

static_assert(SYLPH_LVIS_MATCH_SLICE_BYTES == LVIS_MATCH_SLICE_BYTES && SYLPH_LVIS_MATCH_MAX_DETS == LVIS_MATCH_MAX_DETS,
              "include/sylph_hip.h and csrc/kernels.h state the same LVIS bounds");

static_assert(SYLPH_COCO_MATCH_TILE_GT == COCO_MATCH_TILE_GT && SYLPH_COCO_ACC_CHUNK == COCO_ACC_CHUNK,
              "include/sylph_hip.h and csrc/kernels.h state the same bounds");

extern "C" {

/* see include/sylph_hip.h */
int sylph_coco_match_tile_gt(int max_det) {
  if (max_det <= 0 || max_det > COCO_MATCH_MAX_DETS) return -1;
  return coco_match_tile_gt(max_det);
}

/* see include/sylph_hip.h */
int sylph_coco_match(sylph_ctx* c, int n_det, const float* det_rows, int n_pairs, int n_cat, const int* det_off, const double* gt_box,
                     const double* gt_area, const int* gt_crowd, const int* gt_off, int max_gt, int n_thr, const double* iou_thr, int n_area,
                     const double* area_rng, int max_det, unsigned char* gt_scratch, unsigned long long* matched, unsigned long long* ignored,
                     int* npig) {
  if (n_det < 0 || n_pairs <= 0 || n_cat <= 0 || n_pairs % n_cat != 0) return fail("sylph_coco_match: bad sizes (n_pairs = images x categories)");
  if (n_thr <= 0 || n_area <= 0 || n_area > 4 || n_thr * n_area > COCO_MATCH_LANES)
    return fail("sylph_coco_match: " + std::to_string(n_area) + " area ranges x " + std::to_string(n_thr) + " thresholds; at most 4 ranges and " +
                std::to_string(COCO_MATCH_LANES) + " combinations (one mask bit each)");
  if (max_det <= 0 || max_det > COCO_MATCH_MAX_DETS)
    return fail("sylph_coco_match: max_det " + std::to_string(max_det) + " is outside 1 .. COCO_MATCH_MAX_DETS = " + std::to_string(COCO_MATCH_MAX_DETS));
  if (max_gt < 0) return fail("sylph_coco_match: max_gt < 0");
  if (!det_off || !gt_off || !iou_thr || !area_rng || !npig) return fail("sylph_coco_match: a device table is NULL");
  if (n_det > 0 && (!det_rows || !matched || !ignored)) return fail("sylph_coco_match: a detection buffer is NULL");
  if (max_gt > 0 && (!gt_box || !gt_area || !gt_crowd)) return fail("sylph_coco_match: a ground-truth buffer is NULL");
  if (max_gt > coco_match_tile_gt(max_det) && !gt_scratch)
    return fail("sylph_coco_match: a pair holds " + std::to_string(max_gt) + " ground-truth boxes, more than the " +
                std::to_string(coco_match_tile_gt(max_det)) + " whose IoU tile fits at max_det " + std::to_string(max_det) +
                " (sylph_coco_match_tile_gt; COCO_MATCH_TILE_GT = " + std::to_string(COCO_MATCH_TILE_GT) +
                " up to max_det 131): gt_scratch_dev (64 bytes per ground-truth box) is needed");
  HIPCHK(hipSetDevice(c->device));
  KCHK(timed_op(c, "coco_match_kernel", 0.0, c->stream, [=](hipStream_t st) {
         return launch_coco_match(n_pairs, n_cat, det_rows, det_off, gt_box, gt_area, gt_crowd, gt_off, max_gt, iou_thr, n_thr, area_rng, n_area,
                                  max_det, gt_scratch, matched, ignored, npig, st);
       }), "coco_match");
  return 0;
}

/* see include/sylph_hip.h */
int sylph_lvis_match_fits(int n_det, int n_gt) {
  if (n_det < 0 || n_gt < 0 || n_det > LVIS_MATCH_MAX_DETS) return -1;
  return lvis_match_fits(n_det, n_gt) ? 1 : 0;
}

/* see include/sylph_hip.h */
int sylph_lvis_match(sylph_ctx* c, int n_det, const float* det_rows, int max_pairs, const int* n_pairs, int n_cat, const int* pair_cat,
                     const int* pair_flags, const int* det_off, const double* gt_box, const double* gt_area, const int* gt_ignore,
                     const int* gt_off, int max_gt, int n_thr, const double* iou_thr, int n_area, const double* area_rng, int max_det,
                     unsigned char* gt_scratch, unsigned long long* matched, unsigned long long* ignored, int* npig) {
  if (n_det < 0 || max_pairs <= 0 || n_cat <= 0) return fail("sylph_lvis_match: bad sizes (n_det >= 0, max_pairs > 0, n_cat > 0)");
  if (n_thr <= 0 || n_area <= 0 || n_area > 4 || n_thr * n_area > COCO_MATCH_LANES)
    return fail("sylph_lvis_match: " + std::to_string(n_area) + " area ranges x " + std::to_string(n_thr) + " thresholds; at most 4 ranges and " +
                std::to_string(COCO_MATCH_LANES) + " combinations (one mask bit each)");
  if (max_det <= 0 || max_det > LVIS_MATCH_MAX_DETS)
    return fail("sylph_lvis_match: max_det " + std::to_string(max_det) + " (detections per image, the most a pair can hold) is outside 1 .. " +
                "LVIS_MATCH_MAX_DETS = " + std::to_string(LVIS_MATCH_MAX_DETS));
  if (max_gt < 0) return fail("sylph_lvis_match: max_gt < 0");
  if (!n_pairs || !pair_cat || !pair_flags || !det_off || !gt_off || !iou_thr || !area_rng || !npig)
    return fail("sylph_lvis_match: a device table is NULL");
  if (n_det > 0 && (!det_rows || !matched || !ignored)) return fail("sylph_lvis_match: a detection buffer is NULL");
  if (max_gt > 0 && (!gt_box || !gt_area || !gt_ignore)) return fail("sylph_lvis_match: a ground-truth buffer is NULL");
  if (!lvis_match_fits(max_det, max_gt) && !gt_scratch)
    return fail("sylph_lvis_match: a pair of " + std::to_string(max_det) + " detections and " + std::to_string(max_gt) +
                " ground-truth boxes does not fit a wave's slice of " + std::to_string(LVIS_MATCH_SLICE_BYTES) +
                " bytes (sylph_lvis_match_fits): gt_scratch_dev (64 bytes per ground-truth box) is needed");
  HIPCHK(hipSetDevice(c->device));
  KCHK(timed_op(c, "lvis_match_kernel", 0.0, c->stream, [=](hipStream_t st) {
         return launch_lvis_match(max_pairs, n_pairs, n_cat, det_rows, det_off, pair_cat, pair_flags, gt_box, gt_area, gt_ignore, gt_off, iou_thr,
                                  n_thr, area_rng, n_area, max_det, gt_scratch, matched, ignored, npig, st);
       }), "lvis_match");
  return 0;
}

/* see include/sylph_hip.h */
int sylph_coco_accumulate(sylph_ctx* c, int n_det, const float* score, const int* rank, const unsigned long long* matched,
                          const unsigned long long* ignored, int n_cat, const int* cat_off, const int* npig, int n_thr, int n_rec,
                          const double* rec_thr, int n_area, int n_maxdet, const int* max_dets, double* precision, double* recall, double* scores) {
  if (n_det < 0 || n_cat <= 0 || n_maxdet <= 0) return fail("sylph_coco_accumulate: bad sizes");
  if (n_thr <= 0 || n_thr > COCO_MAX_THRESHOLDS || n_area <= 0 || n_area > 4 || n_thr * n_area > COCO_MATCH_LANES)
    return fail("sylph_coco_accumulate: at most " + std::to_string(COCO_MAX_THRESHOLDS) + " IoU thresholds, 4 area ranges and " +
                std::to_string(COCO_MATCH_LANES) + " combinations");
  if (n_rec <= 0 || n_rec > COCO_MAX_REC_THRESHOLDS)
    return fail("sylph_coco_accumulate: n_rec " + std::to_string(n_rec) + " is outside 1 .. " + std::to_string(COCO_MAX_REC_THRESHOLDS));
  if ((long)n_cat * n_area * n_maxdet >= (1L << 31)) return fail("sylph_coco_accumulate: categories x areas x maxDets does not fit a block index");
  if (!cat_off || !npig || !rec_thr || !max_dets || !precision || !recall || !scores) return fail("sylph_coco_accumulate: a device buffer is NULL");
  if (n_det > 0 && (!score || !rank || !matched || !ignored)) return fail("sylph_coco_accumulate: a detection buffer is NULL");
  HIPCHK(hipSetDevice(c->device));
  KCHK(timed_op(c, "coco_accumulate_kernel", 0.0, c->stream, [=](hipStream_t st) {
         return launch_coco_accumulate(score, rank, matched, ignored, n_cat, cat_off, npig, n_thr, n_rec, rec_thr, n_area, n_maxdet, max_dets,
                                       precision, recall, scores, st);
       }), "coco_accumulate");
  return 0;
}

}  // extern "C"
