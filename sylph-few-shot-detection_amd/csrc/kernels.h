// Launcher prototypes and small device-table structs shared by the translation units.
#pragma once
#include "common.h"

namespace sylph {

struct ImageDesc { const float* ptr; int h, w; };   // one (3,h,w) fp32 plane-major image on device
struct RowSeg { int row0, nrows; };                 // a run of rows (one GroupNorm sample)
// one uint8 HWC image of the fused resize input pipeline: source, target size, offsets of its tables in the int table buffer
struct ResizeDesc { const unsigned char* src; int h, w, new_h, new_w; int hb_off, hk_off, vb_off, vk_off, ksh, ksv; };
// one VIEW of a device-resident uint8 HWC source (sylph_preprocess_views): the crop (x0, y0) + (cw, ch) of a source whose rows are
// `pitch` pixels apart, resized to new_h x new_w with the tables of (cw -> new_w) / (ch -> new_h), mirrored afterwards when flip != 0
struct ViewDesc { const unsigned char* src; int pitch, x0, y0, new_h, new_w, flip; int hb_off, hk_off, vb_off, vk_off, ksh, ksv; };
// one view of sylph_merge_views: its source, the crop origin and width in source pixels, mirrored or not
struct MergeView { int src; float x0, y0, w; int flip; };
// rows one source's views may hold together (max_in x its views): keys, boxes, classes and kept positions of the whole pool live in LDS
constexpr int MERGE_POOL_CAP = 4096;

constexpr int GN_ROWS_PER_CHUNK = 256;
// Block cap of the head's persistent streaming kernels -- gn_logits_kernel<false / true> and gn_taps_kernel (head_fused.hip),
// logits_scan_kernel (detect.hip): each launches head_stream_grid(n_tiles) = min(n_tiles, HEAD_STREAM_MAX_BLOCKS) blocks over the 128-row tile table, so above the
// cap a wave takes several row groups and carries its coefficient table, code fragments and candidate list from one to the next.
// tests/test_head_sweeps_gpu.py pins that regime at small shapes and restates the value: change both together.
constexpr int HEAD_STREAM_MAX_BLOCKS = 2048;
inline int head_stream_grid(int n_tiles) { return n_tiles < HEAD_STREAM_MAX_BLOCKS ? n_tiles : HEAD_STREAM_MAX_BLOCKS; }  // one block = one 128-row tile per sweep
// a GroupNorm sample (= conv segment) whose statistics were left by the conv epilogue as per-M-tile partials
struct GnSeg { int row0, nrows, tile0, ntiles; };

// One (image, FPN level) slab of the head outputs, for decode.
struct DecodeSeg {
  int row0;        // first row in logits / pred buffers
  int nloc;        // H*W
  int W;           // feature width
  int stride;      // FPN stride
  int level;       // FPN level index (0..)
  int image;       // batch index
  unsigned loc_base;  // sum_{l'<l} nloc_l'; global candidate ordinal = (loc_base + loc) * N + cls
  int ncls;        // 0: N = DecodeCfg::num_classes; mixed-episode head: N of the image's episode, negated where the fused scan has left its candidates
  int cls0;        // first logits column of the segment's classes (a multiple of 4; 0 except in a code-sets table)
  int slot;        // output slot: pool, sorted candidates and detections are per slot.  = image, except in a code-sets table, where the
                   // slot of (set g, image i) is g * B + i and `image` keeps indexing the image-size table
};

struct DecodeCfg {
  int num_classes;     // N
  int logits_ld;       // row stride of logits
  float pre_nms_thresh;
  int pre_nms_topk;
  float nms_thresh;
  int post_nms_topk;
  int thresh_with_ctr;
  int quality_mode;    // 0 ctrness, 1 iou, 2 sqrt(iou*ctrness)
  int cand_cap;        // per-(image,level) candidate capacity
  int pool_cap;        // per-image sorted pool capacity (power of two, >= levels*topk)
  int nlevels;
  int max_out;         // per-image output capacity
};

// pre-NMS top-k workspace (detect.hip)
constexpr int SEL_BINS = 4096;  // key >> 19 of a non-negative float: 8 exponent bits + the top 4 mantissa bits
constexpr int SEL_TIE = 4096;   // composites of the boundary bin kept for the exact selection
constexpr int SEL_STATE = 4;    // per segment: [0] boundary-bin candidates written, [1] boundary bin, [2] how many of it are kept, [3] its population
constexpr int SEL_WS = SEL_BINS + SEL_STATE;  // unsigned words of select workspace per segment (zeroed per call)

struct DecodeBuffers {
  // scan
  unsigned* cand_key;   // [nseg][cand_cap]   float bits of cls*quality
  unsigned* cand_idx;   // [nseg][cand_cap]   loc*N + cls
  unsigned* cand_count; // [nseg]
  // select (pre-NMS top-k)
  unsigned* sel_ws;             // [nseg][SEL_WS]   score histogram + state, zeroed per call
  unsigned long long* sel_tie;  // [nseg][SEL_TIE]  composites of the bin the k-th largest falls in
  // pool (per image)
  unsigned long long* pool_key;  // [B][pool_cap]  (sqrt-score bits << 32) | ~ordinal
  unsigned* pool_count;          // [B]
  // sorted candidates
  float* s_box;      // [B][pool_cap][4]
  float* s_score;    // [B][pool_cap]
  int* s_cls;        // [B][pool_cap]
  int* s_level;      // [B][pool_cap]
  float* s_loc;      // [B][pool_cap][2]
  unsigned* s_ord;   // [B][pool_cap]
  int* status;       // [2] [0] bit0: candidate overflow, bit1: output truncated (handed to the caller and cleared by nms_kernel); [1] nms blocks done
};

struct ImageOut { float sx, sy, out_w, out_h; };  // postprocess scale + clip box per image

// elementwise.hip
int launch_preprocess(DType dt, const ImageDesc* imgs_dev, void* out, int B, int H, int W, const float* mean,
                      const float* stdv, hipStream_t s);
int launch_resize_preprocess(DType dt, const ResizeDesc* descs_dev, const int* tab_dev, void* out, int B, int H, int W,
                             const float* mean, const float* stdv, int rgb_input, hipStream_t s);
int launch_view_preprocess(DType dt, const ViewDesc* descs_dev, const int* tab_dev, void* out, int B, int H, int W,
                           const float* mean, const float* stdv, int rgb_input, hipStream_t s);
int launch_export_input(DType dt, const void* x, float* out, int B, int H, int W, hipStream_t s);
// merge_views.hip: one block per source; src_off [n_src + 1] / src_views: the views of every source in ascending order; pool_max: the
// largest max_in x views of a source (<= MERGE_POOL_CAP); status (one int) is cleared here and receives 2 when a source was truncated
int launch_merge_views(int n_src, const int* src_off, const int* src_views, const MergeView* views, int max_views_per_src, int pool_max,
                       int max_in, const float* boxes, const float* scores, const int* classes, const int* counts, float nms_thresh,
                       int post_nms_topk, int max_out, float* out_boxes, float* out_scores, int* out_classes, int* out_view, int* out_row,
                       int* out_counts, int* status, hipStream_t s);
// merge_views_large.hip: the same merge with the pool in a caller's workspace (sylph_merge_views_large).  Rows one source's views may hold
// together.  It bounds the workspace, not the time: a one-class source with K = 0 is one serial, roughly quadratic walk of
// pool / MERGE_LARGE_CHUNK chunks (DESIGN: 6.1 s at 262 144 rows, about 100 s at the cap by extrapolation, not measured).
constexpr int MERGE_LARGE_POOL_CAP = 1048576;
constexpr int MERGE_LARGE_SORT_TILE = 2048;  // keys one block sorts in LDS; the sorted length is a power of two of at least one tile
constexpr int MERGE_LARGE_CHUNK = 64;        // boxes per step of a segment's walk: the chunk of nms_walk.h
constexpr int MERGE_LARGE_KEPT_LDS = 2048;   // kept boxes of a segment that stay in LDS; later ones spill to the workspace
// merge_large_layout(...) is THE workspace layout -- launch, the host check, sylph_merge_views_large_bytes all call it -- and with `stitch`
// that of sylph_stitch_views, which is never below the large merge's.  bytes = -1: refused (a non-positive argument, or n_views * max_in
// does not fit a row index).  Every part starts 16-byte aligned; an offset of the other layout is 0
struct MergeLargeLayout { long long bytes, rows, P, keys_off, kbox_off, kept_off, ubox_off, meta_off, row_off, outu_off, outc_off, bounds_off; };
inline MergeLargeLayout merge_large_layout(int n_src, int n_views, int max_in, bool stitch = false) {
  MergeLargeLayout L = {-1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (n_src <= 0 || n_views <= 0 || max_in <= 0 || (long long)n_views * max_in >= (1LL << 31)) return L;
  L.rows = (long long)n_views * max_in;
  L.P = MERGE_LARGE_SORT_TILE;
  while (L.P < L.rows) L.P <<= 1;
  const auto up16 = [](long long v) { return (v + 15) / 16 * 16; };
  L.keys_off = 0;                                  // P 128-bit keys
  L.kbox_off = L.keys_off + 16 * L.P;              // rows float4: the kept boxes a segment spills
  long long end = L.kbox_off + 16 * L.rows;
  if (!stitch) {
    L.kept_off = end;                              // rows bytes: kept or not, per sorted position
    end = L.kept_off + up16(L.rows);
  } else {
    L.ubox_off = end;                              // rows float4: the kept boxes' union boxes
    L.meta_off = L.ubox_off + 16 * L.rows;         // rows words: their cut bit, dropped bit and count
    L.row_off = L.meta_off + up16(4 * L.rows);     // rows words: the input row of each
    L.outu_off = L.row_off + up16(4 * L.rows);     // rows float4: per INPUT row, the union box of a survivor
    L.outc_off = L.outu_off + 16 * L.rows;         // rows ints: per input row, 0 or 1 + what the survivor absorbed
    end = L.outc_off + up16(4 * L.rows);
  }
  L.bounds_off = end;                              // n_src x (begin, end) of every source's run of kept rows / survivors
  L.bytes = L.bounds_off + up16(8LL * n_src);
  return L;
}
// status (one int) is cleared here and receives 2 when a source was truncated; K <= 0 keeps every kept box
int launch_merge_views_large(int n_src, int n_views, const MergeView* views, int max_in, const float* boxes, const float* scores,
                             const int* classes, const int* counts, float nms_thresh, int K, int max_out, float* out_boxes, float* out_scores,
                             int* out_classes, int* out_view, int* out_row, int* out_counts, int* status, void* workspace, hipStream_t s);
// merge_views_large.hip: the merge that stitches what tile borders cut (sylph_stitch_views): the keys and sorts of the large merge, a
// segment walk that absorbs cut fragments into their keeper's union box (rule 4a), a second walk over the kept rows (rule 4b).
// StitchView: what rule 0 needs beyond MergeView -- the crop's height and the source's size
struct StitchView { float h, src_w, src_h; };
inline MergeLargeLayout stitch_layout(int n_src, int n_views, int max_in) { return merge_large_layout(n_src, n_views, max_in, true); }
// status as launch_merge_views_large; sviews [n_views]; stitch_thr in (0, 1], border_px >= 0 (the host has checked)
int launch_stitch_views(int n_src, int n_views, const MergeView* views, const StitchView* sviews, int max_in, const float* boxes,
                        const float* scores, const int* classes, const int* counts, float nms_thresh, float stitch_thr, float border_px, int K,
                        int max_out, float* out_boxes, float* out_scores, int* out_classes, int* out_view, int* out_row, int* out_stitched,
                        int* out_counts, int* status, void* workspace, hipStream_t s);
// coco_eval.hip: COCO bbox matching and accumulation (include/sylph_hip.h: sylph_coco_match / sylph_coco_accumulate)
// ground-truth boxes of one (image, category) pair whose D x G float64 IoU tile (D <= max_det) is kept in LDS; a pair with more recomputes
// every IoU where the walk visits it and keeps its matched flags in the caller's scratch.  The bound holds up to max_det = 131; a larger
// max_det shrinks it so that the block's LDS (32 B per detection slot + (8 max_det + 64) B per box) stays within COCO_MATCH_LDS_BYTES:
// coco_match_tile_gt(max_det) is THE bound -- launch, host checks and sylph_coco_match_tile_gt all call it.
// tests/test_coco_eval_gpu.py crosses both the constant and a shrunken bound.
constexpr int COCO_MATCH_TILE_GT = 128;
constexpr int COCO_MATCH_LDS_BYTES = 144 * 1024;  // of the CU's 160 KiB
inline int coco_match_tile_gt(int max_det) {
  const long fit = ((long)COCO_MATCH_LDS_BYTES - 32L * max_det) / (8L * max_det + 64);
  return fit < COCO_MATCH_TILE_GT ? (int)fit : COCO_MATCH_TILE_GT;
}
constexpr int COCO_MATCH_MAX_DETS = 1024;  // maxDets[-1]: the detection boxes of a pair live in LDS
constexpr int COCO_MATCH_LANES = 40;       // (area range, IoU threshold) combinations: one lane and one mask bit each
// rows of a category's segment one block scans per step of coco_accumulate_kernel; longer segments carry their counts from chunk to chunk
constexpr int COCO_ACC_CHUNK = 1024;
constexpr int COCO_MAX_THRESHOLDS = 10;
constexpr int COCO_MAX_REC_THRESHOLDS = 128;
int launch_coco_match(int n_pairs, int K, const float* det, const int* det_off, const double* gt_box, const double* gt_area, const int* gt_crowd,
                      const int* gt_off, int max_gt, const double* iou_thr, int T, const double* area_rng, int A, int max_det,
                      unsigned char* gt_scratch, unsigned long long* matched, unsigned long long* ignored, int* npig, hipStream_t s);
int launch_coco_accumulate(const float* score, const int* rank, const unsigned long long* matched, const unsigned long long* ignored, int K,
                           const int* cat_off, const int* npig, int T, int R, const double* rec_thr, int A, int M, const int* max_dets,
                           double* precision, double* recall, double* scores, hipStream_t s);
// lvis_eval.hip: LVIS (federated) bbox matching over a compacted list of the (image, category) pairs that exist (include/sylph_hip.h:
// sylph_lvis_match); the accumulation is coco_accumulate_kernel with one unbounded maxDet.  One wave per pair, LVIS_MATCH_WAVES waves per
// block, each wave with an LDS slice of LVIS_MATCH_SLICE_BYTES = 36 KiB of its own (4 x 36 KiB = 144 KiB of the CU's 160 KiB).  A pair of D
// detections and G boxes keeps its D x G float64 IoU tile and its G 64-byte state rows in the slice when
// 32 D + G (8 D + 64) <= LVIS_MATCH_SLICE_BYTES (D = 300: 11 boxes, D = 64: 60, D = 1: 511); any other pair recomputes the IoU at every
// visit and keeps its state rows in the caller's scratch.  lvis_match_fits is THE rule: kernel, host check and sylph_lvis_match_fits call it.
constexpr int LVIS_MATCH_WAVES = 4;
constexpr int LVIS_MATCH_SLICE_BYTES = 36 * 1024;
constexpr int LVIS_MATCH_MAX_DETS = 1024;  // detections of one pair (<= max_dets_per_image): their boxes live in the wave's slice, 32 B each
__host__ __device__ inline bool lvis_match_fits(int n_det, int n_gt) {
  return 32L * n_det + (long)n_gt * (8L * n_det + 64) <= (long)LVIS_MATCH_SLICE_BYTES;
}
int launch_lvis_match(int max_pairs, const int* n_pairs, int K, const float* det, const int* det_off, const int* pair_cat, const int* pair_flags,
                      const double* gt_box, const double* gt_area, const int* gt_ignore, const int* gt_off, const double* iou_thr, int T,
                      const double* area_rng, int A, int max_det, unsigned char* gt_scratch, unsigned long long* matched,
                      unsigned long long* ignored, int* npig, hipStream_t s);
int launch_maxpool(DType dt, const void* in, void* out, int B, int H, int W, int C, int Ho, int Wo, hipStream_t s);
int launch_groupnorm(DType dt, void* x, const RowSeg* segs_dev, int nseg, int max_rows, int ld, const float* gamma,
                     const float* beta, float eps, int relu, float* partial, float2* stats, hipStream_t s);
// stem_conv.hip
int launch_stem_conv(const void* x, const void* wp, const float* scale, const float* shift, void* out, int B, int H, int W, int H2,
                     int W2, hipStream_t s);
int launch_gn_logits(const void* x, int ld, const float2* coef, const void* w, const float* bias, int N, float* out, int out_ld,
                     const SegDesc* segs, const int2* tiles, int n_tiles, hipStream_t s);  // head_fused.hip (bf16, N <= 32)
// the same for a batch whose images belong to different episodes: w / bias hold every episode's 32 zero-padded rows, seg_row0[seg] the
// first row of the block of the segment's image
// the 3x3 sibling (CLS_LAYER kernel size 3): w [32][3][3][256] bf16 (launch_pack_codes3x3), zero padding of the normalised tensor
int launch_gn_cond3x3(const void* x, int ld, const float2* coef, const void* w, const float* bias, int N, float* out, int out_ld,
                      const SegDesc* segs, const int2* tiles, int n_tiles, hipStream_t s);
int launch_gn_logits_episodes(const void* x, int ld, const float2* coef, const void* w, const float* bias, const int* seg_row0, float* out,
                              int out_ld, const SegDesc* segs, const int2* tiles, int n_tiles, hipStream_t s);
// several code sets over the same images: nblocks <= GN_SETS_MAX_BLOCKS blocks of 32 packed code rows per pass over the tower output
constexpr int GN_SETS_MAX_BLOCKS = 4;
int launch_gn_logits_sets(const void* x, int ld, const float2* coef, const void* w, const float* bias, int nblocks, float* out, int out_ld,
                          int width, const SegDesc* segs, const int2* tiles, int n_tiles, hipStream_t s);  // head_fused.hip (bf16)
int launch_gn_pred_taps(const void* x, int ld, const float2* coef, const void* w_taps, int cp, const float* bias, int relu_nch, int mul_nch,
                        float* planes_ws, size_t plane_rows, float* out, int out_ld, const SegDesc* segs, const int2* tiles, int n_tiles,
                        hipStream_t s);  // head_fused.hip: last bbox-tower GroupNorm + 3x3 prediction convs (bf16)
// finetune.hip: FCOS classification targets, and loss + gradient of the focal loss with respect to one block of <= 32 class codes (bf16)
struct FcosTargetCfg { int strides[8]; float lo[8], hi[8]; int center_sample; float radius; };  // lo / hi: the level's range of the largest regression target
int launch_fcos_targets(const SegDesc* segs, int nseg, int nlevels, int max_rows, const FcosTargetCfg& cfg, int n_gt, const float* boxes,
                        const int* gt_class, const int* gt_image, int* labels, int* num_pos, hipStream_t s);
constexpr int CLS_GRAD_UNIT_GROUPS = 16;  // 32-row groups behind one partial: fixed by the tile table, so the sums do not depend on the grid
constexpr int CLS_GRAD_PARTIAL = 8256;    // floats per partial: [256][32] dW^T | [32] db | loss, rounded up to 128 bytes
constexpr int CLS_GRAD_FANIN = 64;        // partials added per reduce pass (partial_sum.h)
constexpr int CLS_GRAD_MAX_BLOCKS = 1024;  // one block of four waves per CU and a few to spare; SYLPH_CLS_GRAD_BLOCKS overrides it
int cls_grad_units(int n_tiles);
size_t cls_grad_ws_floats(int n_tiles);
int launch_cls_grad(const void* x, int ld, const float2* coef, const void* w, const float* bias, int nb, int n0, const int* labels, float alpha,
                    float gamma, float* ws, float* loss, int accumulate, float* grad_w, float* grad_b, const SegDesc* segs, const int2* tiles,
                    int n_tiles, hipStream_t s);
// box_finetune.hip: the box-sample bank of a fresh batch (positives in row order: info, targets, normalised 3x3 patches of the bbox tower),
// and loss + gradient of the box / centerness / IoU losses with respect to the box branch (bf16)
inline int box_samples_gx(int max_rows) { return (max_rows + 255) / 256; }  // 256-row blocks per segment: assign [rows], blk [nseg * gx] ints
int launch_box_samples(const void* x, const float2* coef, const SegDesc* segs, int nseg, int nlevels, int max_rows, int rows_per_image,
                       const FcosTargetCfg& cfg, int n_gt, const float* boxes, const int* gt_class, const int* gt_image, int* assign, int* blk,
                       int max_samples, void* patches, float* targets, int* info, int* count, int* status, hipStream_t s);
constexpr int BOX_GRAD_UNIT = 32;          // samples behind one partial: fixed by n, so the sums do not depend on the grid
constexpr int BOX_GRAD_DB = 6 * 2304;      // a partial: [6][2304] dW | [6] db | [8] d scales | [4] sums, rounded up to 128 bytes
constexpr int BOX_GRAD_DS = BOX_GRAD_DB + 8;
constexpr int BOX_GRAD_SUMS = BOX_GRAD_DS + 8;
constexpr int BOX_GRAD_PARTIAL = BOX_GRAD_SUMS + 16;
constexpr int BOX_GRAD_FANIN = 64;         // partials added per reduce pass (partial_sum.h)
constexpr int BOX_GRAD_MAX_BLOCKS = 1024;  // SYLPH_BOX_GRAD_BLOCKS overrides it
int box_grad_units(int n);
size_t box_grad_ws_floats(int n);
int launch_box_grad(int n, const void* patches, const float* targets, const int* info, const float* w, const float* bias, const float* scales,
                    int cout, int nlevels, int quality, int iou_mask, float* ws, float* sums, float* grad_w, float* grad_b, float* grad_scales,
                    float* z_out, float* g_out, hipStream_t s);
int launch_stem_pool(const void* x, const void* wp, const float* scale, const float* shift, void* out, void* trash, int B, int H, int W,
                     int H2, int W2, int H4, int W4, hipStream_t s);
constexpr int STEM_RAW_MAX_BATCH = 512;  // the image table of launch_stem_pool_raw lives in LDS
int launch_stem_pool_raw(const ImageDesc* imgs_dev, const float* mean, const float* stdv, const void* wp, const float* scale,
                         const float* shift, void* out, void* trash, int B, int H, int W, int H2, int W2, int H4, int W4, hipStream_t s);  // stem + max-pool fused (bf16); trash >= 512 x 256 x 16 B
int launch_gn_apply_partials(DType dt, void* x, int ld, int ngroups, const GnSeg* segs_dev, int nseg, int max_rows,
                             const float* partial, float2* stats_ws, const float* gamma, const float* beta, float eps, int relu,
                             hipStream_t s);
int launch_gn_finalize_coef(int ngroups, const GnSeg* segs_dev, int nseg, const float* partial, float2* stats_ws, const float* gamma,
                            const float* beta, float eps, float2* coef, hipStream_t s);
int launch_fill_random(DType dt, void* p, size_t n, unsigned seed, hipStream_t s);
struct CopySeg { int src_row0, dst_row0, nrows; };
int launch_relu_rows(DType dt, const void* src, void* dst, int ld, const CopySeg* segs_dev, int nseg, int max_rows,
                     hipStream_t s);
int launch_import_nchw(DType dt, const float* src, void* dst, int C, int HW, int row0, int ld, hipStream_t s);
int launch_export_nchw(DType dt, const void* src, float* dst, int C, int HW, int row0, int ld, hipStream_t s);
int launch_export_nchw_f32(const float* src, float* dst, int C, int HW, int row0, int ld, int ch0, hipStream_t s);
int launch_pack_codes(DType dt, const float* w, int N, int C, int Npad, void* out, const float* bias, float* bias_pad, float* bias_scan, hipStream_t s);
// 3x3 class codes (N,C,3,3) fp32 -> [Npad][3][3][C] in the compute dtype (pack_conv's layout, DT_F32S: its split hi / lo form), zero
// padding rows; biases as launch_pack_codes pads them
int launch_pack_codes3x3(DType dt, const float* w, int N, int C, int Npad, void* out, const float* bias, float* bias_pad, float* bias_scan,
                         hipStream_t s);
// several episodes' codes in one launch: packed row r takes row src_row[r] of w / bias, or zeros (bias_scan: -inf) where src_row[r] < 0
int launch_pack_codes_episodes(DType dt, const float* w, const int* src_row, int rows, int C, void* out, const float* bias, float* bias_pad,
                               float* bias_scan, hipStream_t s);

// conv_deform.hip: modulated deformable 3x3 conv (DCNv2, deformable FCOS tower layer), 256 -> 256 channels, stride 1, pad 1.
// x: the layer input [rows][256] (storage dtype), om: its offset-conv output [rows][om_ld] fp32 (dy, dx of tap j in 2j, 2j + 1,
// mask logits in 18 .. 26), wt: the conv_igemm weight layout [256][3][3][256] (fp32 in DT_F32 and DT_F32S), out: [rows][256];
// tiles: 128-row tiles of the segments (make_geom), gn_partial: optional [n_mtiles][32][3] GroupNorm partials (n, mean, M2)
struct DeformArgs {
  const void* x;
  const float* om;
  const void* wt;
  const float* bias;
  void* out;
  const void* zeros;  // >= 128 B of zeros
  const SegDesc* segs;
  const int2* tiles;
  float* gn_partial;
  int n_mtiles, om_ld, relu;
};
int launch_conv_deform(DType dt, const DeformArgs& a, hipStream_t s);

// conv_group.hip: grouped 3x3 conv (ResNeXt bottleneck conv2), pad 1, stride 1 / 2, FrozenBN scale / shift (+ ReLU) in the epilogue.
// x [B][Hin * Win][C] -> y [B][Ho * Wo][C] (storage dtype, dense images); wt: conv_group_pack's layout (conv_group_packed_bytes);
// scale / shift: C fp32.  C % 64 == 0, cpg = C / groups a power of two in [4, 64].
struct GroupConvArgs {
  const void* x;
  void* y;
  const void* wt;
  const float* scale;
  const float* shift;
  int B, C, cpg, Hin, Win, Ho, Wo, stride, relu;
};
size_t conv_group_packed_bytes(DType dt, int C, int cpg);
void conv_group_pack(DType dt, const float* w, int C, int cpg, void* out);
int launch_conv_group(DType dt, const GroupConvArgs& a, hipStream_t s);

// conv_dw.hip: the direct convs of the MobileNetV2 bottom-up path, fp32 arithmetic in every storage mode.
// Depthwise 3x3 (pad 1, stride 1 / 2) on dense images x [B][H * W][ld] -> y [B][Ho * Wo][ld], the first C channels of every row:
// y = relu6(scale * conv(clamp(x, 0, 6)) + shift); w fp32 [3][3][C], scale / shift fp32 [C]; C and ld multiples of 8, ld >= C.
struct DwConvArgs {
  const void* x;
  void* y;
  const float *w, *scale, *shift;
  int B, C, ld, H, W, Ho, Wo, stride;
};
int launch_dwconv3x3(DType dt, const DwConvArgs& a, hipStream_t s);
// features.0: 3x3 stride-2 pad-1 conv 3 -> 32 + FrozenBN + ReLU6 on the normalised batch x [B][H][W][4] -> y [B][Ho * Wo][ld], the first C
// channels of every row, C >= 32 (channels >= 32: zeros); C and ld multiples of 8; w fp32 [3][3][4][32] (input channel 3 zero), scale / shift fp32 [32]
struct MbStemArgs {
  const void* x;
  void* y;
  const float *w, *scale, *shift;
  int B, C, ld, H, W, Ho, Wo;
};
int launch_mbv2_stem(DType dt, const MbStemArgs& a, hipStream_t s);

// conv_mbv2.hip: one whole InvertedResidual block per launch, bf16 only; the hidden tensor stays in LDS.
// x [B][H * W][cin_ld] -> y [B][Ho * Wo][cout_ld], the first cin_p / cout_p channels of every row.  w1 bf16 [hid_p][cin_p] (nullptr: t == 1,
// hidden = input, hid_p == cin_p), w2 bf16 [cout_p][hid_p], wd fp32 [3][3][hid_p]; s* / b* the folded FrozenBN scale / shift of the three
// layers.  cin_p and hid_p multiples of 32, cout_p 64 / 128 / 192 / 320; residual: y += x (stride 1, cin_p == cout_p).
struct Mbv2Args {
  const void* x;
  void* y;
  const bf16_t *w1, *w2;
  const float *s1, *b1, *wd, *sd, *bd, *s2, *b2;
  int B, H, W, Ho, Wo, stride, cin_p, cin_ld, hid_p, cout_p, cout_ld, residual;
};
bool conv_mbv2_can_run(const Mbv2Args& a);
int launch_conv_mbv2(const Mbv2Args& a, hipStream_t s);

// detect.hip
// many-way class-conditional conv fused with the scan (detect.hip); x: raw cls-tower output, coef: its GroupNorm (a, b) per
// (segment, channel), w: packed codes [>= 32 * ceil(N/32)][256] bf16, wf_ws: as many bytes of workspace (the codes in MFMA
// fragment order), bias_scan: fp32 biases (zeros without a bias), -inf from class N up to the same row count
// clear_counts: zero the nseg candidate counters first (the mixed-episode head clears once and scans one tile sub-list per episode)
int launch_logits_scan(const void* x, int ld, const float2* coef, const void* w, void* wf_ws, const float* bias_scan,
                       const SegDesc* segs, const int2* tiles, int n_tiles, const float* pred, int pred_ld, const DecodeCfg& cfg,
                       const DecodeBuffers& buf, int nseg, bool clear_counts, hipStream_t s);
// B: output slots (images; sets x images for a code-sets table), nseg = B * levels segments, slot-major
int launch_decode(const DecodeCfg& cfg, const DecodeSeg* segs_dev, int nseg, int max_nloc, int B, int nw_bound,
                  const float* logits, const float* pred, int pred_ld, const DecodeBuffers& buf,
                  const ImageOut* img_out_dev, float* out_boxes, float* out_scores, int* out_classes,
                  int* out_levels, float* out_locations, int* out_cand, int* out_counts, int* status_out, bool candidates_ready, hipStream_t s);

// codegen.hip
struct LevelDesc { int row0; int H, W; float scale; };  // per (image, level): rows of the feature pyramid
// row r: box r on image roi_image_dev[r] of the batch (lv_dev: an entry per (image, level))
int launch_roi_align(DType dt, const void* feats, int ld, const LevelDesc* lv_dev, int nlevels, const float* boxes_dev,
                     const int* roi_image_dev, int R, int out_size, void* out, hipStream_t s);
constexpr int TAIL_MAX_LEN = 16384;  // longest segment of a tail / shot-combine launch: 64 KiB of shot weights in LDS
// one code per segment of the ROI list: seg_dev[j] = {first row, rows}; max_len = the longest segment (sizes the LDS weight table)
int launch_codegen_tail(const float* conv_out, int conv_ld, const float* aux_out, int aux_ld, int ib, int iw, int is, const int2* seg_dev,
                        int n_seg, int max_len, int npos, int C, int ksize, int bias_l2_norm, float* code_out, float* wnorm_out, hipStream_t s);
int launch_normalize_codes(float* codes, int ncodes, int C, int ksize, const float* gn_gamma, const float* gn_beta, int post_norm,
                           int l2_norm, float conv_scale, float bias_scale, float bias_prior, const float* weight_norm,
                           hipStream_t s);
int launch_reduce_codes(const float* rows, int n, int ld, float* out, int num_classes, int divide_by_acc, hipStream_t s);

// roi_encoder.hip
struct MsCamWeights {  // fp32 device pointers: conv1x1 256->64, GN(32,64), conv1x1 64->256, GN(32,256); local / global
  const float *l_w1, *l_b1, *l_g1, *l_be1, *l_w2, *l_b2, *l_g2, *l_be2;
  const float *g_w1, *g_b1, *g_g1, *g_be1, *g_w2, *g_b2, *g_g2, *g_be2;
};
int launch_adaptive_context(DType dt, const void* feats, int ld, const LevelDesc* lv_dev, int nlevels, int S,
                            int out_size, float* ctx, hipStream_t s);
int launch_mscam(DType dt, const float* ctx, const int* ctx_row_dev, void* x, int R, const MsCamWeights& w, hipStream_t s);
int launch_linear(int x_is_bf16, const void* x, int ldx, int S, const float* W, const float* b, int K, int O, float* y,
                  int ldy, int relu, float add, hipStream_t s);
int launch_add_layernorm(float* x, const float* r, int S, const float* gamma, const float* beta, hipStream_t s);
int launch_mean_tokens(const float* x, const int2* seg_dev, int n_seg, float* out, hipStream_t s);

// shot_bank.hip: the per-shot rows of the support path ([R][row_ld] fp32, row_ld >= C k^2 + 4 resp. 256) and the code of any gathered
// list of them: segment j = rows idx_dev[seg_dev[j].x + i], i < seg_dev[j].y; n = C k^2 code values per row
int launch_shot_pool(const float* conv_out, int conv_ld, const float* aux_out, int aux_ld, int ib, int iw, int is, int R, int npos, int C,
                     int ksize, int bias_l2_norm, float* rows, int row_ld, hipStream_t s);
int launch_shot_token_rows(const float* tok, int R, float* rows, int row_ld, hipStream_t s);
int launch_shot_combine(const float* rows, int row_ld, const int* idx_dev, const int2* seg_dev, int n_seg, int max_len, int n, int has_b,
                        int has_w, int has_s, float* code_out, float* wnorm_out, hipStream_t s);
int launch_shot_mean_tokens(const float* rows, int row_ld, const int* idx_dev, const int2* seg_dev, int n_seg, float* out, hipStream_t s);

// codegen_train.hip: training-mode forward of the CodeGenerator on a bank of ROI rows and its backward down to every parameter
constexpr int CGT_MAX_TOWER = 30;    // TOWER_LAYERS entries
constexpr int CGT_UNIT_SHOTS = 4;    // shots behind one weight-gradient partial: fixed by M, so the sums do not depend on the grid
constexpr int CGT_FANIN = 8;         // partials added per reduce pass
constexpr int CGT_MAX_BLOCKS = 4096; // SYLPH_CODEGEN_TRAIN_BLOCKS overrides it
struct CgtCfg { int L, has_bias, post_norm, l2_norm, has_conv_scale; float prior; };
// offsets (floats) of the trainable tensors in the flat parameter / gradient vector; -1: the config has no such tensor
struct CgtParams { long tw[CGT_MAX_TOWER], tb[CGT_MAX_TOWER], tg[CGT_MAX_TOWER], tbe[CGT_MAX_TOWER], cw, cb, bw, bb, pg, pb, cs, bs, total; };
// offsets (bytes) of the workspace's parts
struct CgtWs {
  size_t idx, seg, wf[CGT_MAX_TOWER], wd[CGT_MAX_TOWER], wh, wht, wb, y[CGT_MAX_TOWER], st[CGT_MAX_TOWER], x[CGT_MAX_TOWER], xsum, c, rb, code_raw,
      bias_raw, dcode_raw, dbias_raw, tpg, tpb, tpcs, tpbs, dc, drb, dxsum, dxa, dya, gsg, gsb, gsd, part, total;
  int units, passes;
};
void cgt_param_layout(const CgtCfg& cfg, CgtParams* p);
void cgt_workspace(const CgtCfg& cfg, int M, int n_seg, CgtWs* w);
size_t cgt_debug_floats(const CgtCfg& cfg, int M, int n_seg);
// rows: the bank, (n_rows, 49, 256) bf16; ws: cgt_workspace bytes whose idx (M ints) and seg (n_seg int2 {first shot, shots}) are filled
int launch_cgt_forward(const CgtCfg& cfg, const float* params, const void* rows, int M, int n_seg, char* ws, float* codes_out, hipStream_t s);
int launch_cgt_backward(const CgtCfg& cfg, const float* params, const void* rows, int M, int n_seg, char* ws, const float* grad_codes,
                        float* grad_out, float* debug_out, hipStream_t s);

}  // namespace sylph
