// Internal declarations shared by the host-side translation units of libsylph_hip.so (api_*.hip): the context, the per-batch-shape
// execution plan, the packed layer records, the plan-building helpers.  Not part of the C ABI (include/sylph_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>
#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/sylph_hip.h"
#include "common.h"
#include "kernels.h"
#include "res3_pair_tiles.h"

using namespace sylph;
namespace sylph_host {
int fail(const std::string& m);  // sets sylph_last_error() of this thread, returns 1
}
using sylph_host::fail;
// collective.hip
hipStream_t sylph_internal_stream(sylph_ctx* c);
int sylph_internal_fail(const std::string& m);
int sylph_internal_code_ksize(sylph_ctx* c);
#define HIPCHK(x)                                                                                  \
  do {                                                                                             \
    hipError_t e_ = (x);                                                                           \
    if (e_ != hipSuccess) return fail(std::string(#x) + ": " + hipGetErrorString(e_));             \
  } while (0)
#define RET(x)                     \
  do {                             \
    int r_ = (x);                  \
    if (r_ != 0) return r_;        \
  } while (0)
// build step of plan P: its allocations belong to P; a failed build releases the whole plan so that a retry starts clean
#define BUILD(x, P)                                  \
  do {                                               \
    int r_ = (x);                                    \
    if (r_ != 0) { drop_plan(c, (P)); return r_; }   \
  } while (0)
#define KCHK(x, what)                                                                              \
  do {                                                                                             \
    int r_ = (x);                                                                                  \
    if (r_ != 0) return fail(std::string(what) + ": launch failed (" + std::to_string(r_) + ")");  \
  } while (0)

static inline uint16_t f2bf_host(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

// The SYLPH_* environment overrides of the host units ("knobs"): every one is declared here and read through knob_env alone.  (Two more are
// read inside kernel units, next to the launch they steer: SYLPH_CONV_BN64_MAX in conv_igemm.hip, SYLPH_SCAN_BLOCKS in detect.hip.)
// Read time: ONCE = at first use, then fixed for the process; LIVE = at every call of the accessor, by the caller named in the row.
namespace sylph_host {
long knob_env(const char* name, long dflt);  // api_core.hip: the value of an integer environment variable, dflt when it is not set
namespace knob {
#define SYLPH_KNOB_ONCE(fn, name, dflt) inline int fn() { static const int v = (int)knob_env(name, dflt); return v; }
#define SYLPH_KNOB_LIVE(fn, name, dflt) inline int fn() { return (int)knob_env(name, dflt); }
// conv routes (pick_conv_route): 0 off, 1 where it pays, 2 wherever the kernel can run
SYLPH_KNOB_ONCE(conv_hpipe, "SYLPH_CONV_HPIPE", 1)
SYLPH_KNOB_ONCE(conv_halo, "SYLPH_CONV_HALO", 1)
SYLPH_KNOB_ONCE(conv_pw, "SYLPH_CONV_PW", 1)
SYLPH_KNOB_ONCE(conv_spw, "SYLPH_CONV_SPW", 1)
SYLPH_KNOB_ONCE(conv_nbuf2, "SYLPH_CONV_NBUF2", 1)           // 0: one LDS stage in the 64-row tiles of conv_igemm
SYLPH_KNOB_ONCE(conv_nbuf3_max, "SYLPH_CONV_NBUF3_MAX", 400)  // launches of at most this many tiles take three stages (0: two everywhere)
SYLPH_KNOB_ONCE(split_k, "SYLPH_SPLIT_K", 1)                 // 0 off, 1 small launches of deep-K layers, 2 every layer of >= 8 K slices
SYLPH_KNOB_ONCE(split_t1, "SYLPH_SPLIT_T1", 64)              // split K up to this many tiles (>= 32 K slices) ...
SYLPH_KNOB_ONCE(split_t2, "SYLPH_SPLIT_T2", 64)              // ... and below this many (>= 64 K slices)
// block routes (pick_conv3_route, pick_block_route, pick_stem_route)
SYLPH_KNOB_ONCE(conv_rw3, "SYLPH_CONV_RW3", 1)               // 0 off, 1 launches of at least 256 x 120 positions, 2 any launch
SYLPH_KNOB_LIVE(conv_rw64, "SYLPH_CONV_RW64", 1)             // 0 off, 1 launches of at least RW64_MIN_PATCHES patches, 2 any launch; per pick
                                                             // (= per build: one process can build both)
SYLPH_KNOB_ONCE(fuse_bottleneck, "SYLPH_FUSE_BOTTLENECK", 1)  // 0: the res2 blocks as conv chains
SYLPH_KNOB_ONCE(bk_strided_tail, "SYLPH_BK_STRIDED_TAIL", 1)  // 0: the last res2 block computes every position
SYLPH_KNOB_ONCE(block_pair, "SYLPH_BLOCK_PAIR", 1)           // res3 identity blocks: conv3 + residual and the next block's conv1 in one launch
                                                             // (conv_spw_pair.hip): 0 off, 1 launches whose conv3 would take conv_spw (512 M tiles of 128 rows), 2 any launch
SYLPH_KNOB_ONCE(stem_kernel, "SYLPH_STEM_KERNEL", 1)         // 0: the stem through conv_igemm
SYLPH_KNOB_ONCE(fuse_stem_pool, "SYLPH_FUSE_STEM_POOL", 1)   // 0: stem_conv + maxpool as two launches
SYLPH_KNOB_LIVE(mbv2_fused, "SYLPH_MBV2_FUSED", 1)           // MobileNetV2 blocks as one conv_mbv2 launch, bf16: 0 off, 1 the block shapes where it beats
                                                             // the three-launch chain (pick_mbv2_route), 2 wherever it can run; per pick (= per build)
// streams and fusions of the FPN / head
SYLPH_KNOB_ONCE(head_streams, "SYLPH_HEAD_STREAMS", 1)       // 0 one stream, 1 two for small batches (FPN top and bbox tower on the side stream), 2 always two
SYLPH_KNOB_ONCE(gn_fuse, "SYLPH_GN_FUSE", 1)                 // 0: every tower GroupNorm as its own apply pass
SYLPH_KNOB_ONCE(fuse_gn_logits, "SYLPH_FUSE_GN_LOGITS", 1)   // 0: the head ops apply the last cls GroupNorm themselves
SYLPH_KNOB_LIVE(gn_cond3x3, "SYLPH_GN_COND3X3", 0)          // 1: 3x3 class codes, bf16, N <= 32 through gn_cond3x3_kernel (off: it does not beat apply + conv_igemm yet); per head call
SYLPH_KNOB_ONCE(fuse_scan, "SYLPH_FUSE_SCAN", 1)             // 0 never, 1 more than 32 classes, 2 any class count
SYLPH_KNOB_LIVE(fuse_preprocess, "SYLPH_FUSE_PREPROCESS", 1)  // 0: a normalised copy of the batch; per sylph_preprocess call
SYLPH_KNOB_LIVE(fuse_shortcut, "SYLPH_FUSE_SHORTCUT", 1)     // 0: conv3 and the projection shortcut as two convs; per sylph_finalize_weights /
                                                             // per bottleneck parity entry call
// plan cache, per sylph_ctx_create
SYLPH_KNOB_LIVE(max_plans, "SYLPH_MAX_PLANS", 32)            // cached plans per context (at least 2)
inline long plan_bytes_mb() { return knob_env("SYLPH_PLAN_BYTES_MB", LONG_MIN); }  // workspace budget in MiB; not set (LONG_MIN here): 60 % of the device
#undef SYLPH_KNOB_ONCE
#undef SYLPH_KNOB_LIVE
}  // namespace knob
}  // namespace sylph_host

typedef std::function<int(hipStream_t)> OpFn;

struct HostTensor {
  std::vector<float> data;
  std::vector<int64_t> shape;
};

struct ConvLayer {
  void* w = nullptr;       // packed [Cout_pad][KH][KW][Cin]
  float* scale = nullptr;  // device, Cout_pad (may be null)
  float* shift = nullptr;
  int Cin = 0, Cout = 0, Cout_pad = 0, KH = 1, KW = 1;
  int groups = 1;          // > 1: grouped 3x3 conv (ResNeXt conv2), w in conv_group_pack's layout, scale / shift Cout floats
};
struct GNLayer {
  float* gamma = nullptr;
  float* beta = nullptr;
};

struct Plan;

// A query record (sylph_record_store): what the towers left for one batch, in ONE device allocation of the context that made it -- not a
// plan's, so plan eviction does not touch it.  Nothing that scores a record writes into it.
struct sylph_record {
  sylph_ctx* owner = nullptr;
  int device = 0;
  DType dt = DT_BF16;
  int tower_norm = 0, nlevels = 0, strides[8] = {0}, code_ksize = 1;  // the sylph_config fields a record's layout and meaning depend on
  int B = 0, H = 0, W = 0;
  uint64_t box_stamp = 0;            // sylph_ctx::box_stamp when the record was stored: its pred rows come from that box branch
  std::vector<int> img_h, img_w;
  void* base = nullptr;              // the allocation: feat | pred | coef | partial, each at a multiple of 256 bytes
  const void* feat = nullptr;        // cls tower output [B * Ltot][256]: un-normalised where the last GroupNorm is deferred (coef != nullptr)
  const float* pred = nullptr;       // [B * Ltot][8]
  const float2* coef = nullptr;      // deferred GroupNorm: (a, b) per (segment, channel) -- what the streaming kernels read
  const float* partial = nullptr;    // ... and the conv epilogue's per-tile partials, which the stand-alone apply reads
  size_t feat_bytes = 0, pred_bytes = 0, coef_bytes = 0, partial_bytes = 0;
  int64_t bytes = 0;
};

// where the class-conditional kernels and the decode read the towers' outputs of the current batch: the plan's own buffers, or a query
// record's in place (api_head.hip: run_towers)
struct TowerSrc {
  const void* feat = nullptr;
  const float2* coef = nullptr;
  const float* pred = nullptr;
};

// the deferred last GroupNorm of a tower, as add_gn_from_partials leaves it: the coefficient table and the per-tile partials behind it
struct GnDeferred {
  const float2* coef = nullptr;
  size_t coef_bytes = 0;
  const float* partial = nullptr;
  size_t partial_bytes = 0;
};

// Pillow's precompute_coeffs + normalize_coeffs_8bpc for the BILINEAR filter (libImaging/Resample.c), in double like the
// original: per output index the first input index, the tap count and `ksize` 22-bit fixed-point weights.
struct PilCoeffs {
  int ksize = 0;
  std::vector<int> bounds;  // [out][2] = (first, count)
  std::vector<int> kk;      // [out][ksize]
};


struct sylph_ctx {
  int device = 0;
  DType dt = DT_BF16;
  hipStream_t stream = nullptr;
  sylph_config cfg;
  bool finalized = false;
  int64_t bytes = 0;
  std::vector<void*> allocs;
  std::map<std::string, HostTensor> host_w;
  // packed model
  ConvLayer stem;  // 7x7 s2 stem packed for the implicit-GEMM stem loader
  void* stem_wp = nullptr;  // bf16 [64][7][8][4] for the dedicated stem kernel (stem_conv.hip)
  struct Block {
    ConvLayer c1, c2, c3, sc, c3sc;
    bool has_sc = false, fused_sc = false;
    bool basic = false;  // detectron2 BasicBlock (R-18 / R-34): c1, c2 are 3x3 convs, no c3, a shortcut only where the width changes
  };
  std::vector<std::vector<Block>> stages;  // res2..res5
  // MobileNetV2 bottom-up (cfg.mobilenet; api_weights.hip make_mbv2_block): one InvertedResidual block.  Every channel count is computed
  // padded to mbv2_pad() channels -- zero weights, scales and shifts, so pad channels are exactly zero in every tensor -- in rows of
  // mbv2_ld() elements.
  struct MbBlock {
    int cin = 0, t = 1, cout = 0, stride = 1;  // logical: hidden = t * cin; the input is added when stride == 1 && cin == cout
    int cin_p = 0, hid_p = 0, cout_p = 0;      // channels as computed (mbv2_pad)
    int cin_ld = 0, hid_ld = 0, cout_ld = 0;   // row pitch of the input, the two hidden tensors and the output (mbv2_ld)
    ConvLayer exp, proj;                       // 1x1 expand (t != 1) and 1x1 linear projection, FrozenBN folded
    float *dw_w = nullptr, *dw_scale = nullptr, *dw_shift = nullptr;  // depthwise 3x3: fp32 [3][3][hid_p] (bf16 mode: bf16-rounded values), [hid_p]
    bf16_t *fw1 = nullptr, *fw2 = nullptr;     // bf16 mode, for conv_mbv2.hip: expand [hid_p][cin_p] (t != 1) and projection [cout_p][hid_p], row-major
    bool residual() const { return stride == 1 && cin == cout; }
  };
  std::vector<MbBlock> mb_blocks;              // features.1 .. features.17
  float *mb_stem_w = nullptr, *mb_stem_scale = nullptr, *mb_stem_shift = nullptr;  // features.0: fp32 [3][3][4][32], [32]
  ConvLayer fpn_lat[3], fpn_out[3], p6, p7;  // index 0..2 = stage 3..5
  std::vector<ConvLayer> cls_tower, box_tower, share_tower;  // share_tower: MODEL.FCOS.NUM_SHARE_CONVS layers in front of both
  std::vector<GNLayer> share_gn;
  std::vector<GNLayer> cls_gn, box_gn;
  ConvLayer cls_off, box_off;  // MODEL.FCOS.USE_DEFORMABLE: offset conv of the last cls / bbox tower layer (27 channels; Cout == 0: plain tower)
  ConvLayer pred;  // bbox_pred(4) + ctrness(1) + iou_overlap(1)
  ConvLayer cls_logits;  // the base detector's own classifier (fcos.py:418-427), 1x1 or 3x3, when the checkpoint carries it
  bool has_cls_logits = false;
  void* pred_taps = nullptr;  // bf16 [64][256]: row kh * sw + kw * Cout + n = pred weight W[n][kh][kw][:] (head_fused.hip), bf16 mode only
  std::vector<float> level_scales;
  std::vector<ConvLayer> cg_tower;
  std::vector<GNLayer> cg_gn;
  ConvLayer cg_cls, cg_bias;  // cg_bias: the 1-channel heads stacked on Cout: [bias][shot weight][class scale] (those the config has)
  int cg_naux = 0, cg_ib = -1, cg_iw = -1, cg_is = -1;  // channel of each head in cg_bias's output (-1: absent)
  GNLayer cg_post;
  float cg_conv_scale = 1.f, cg_bias_scale = 1.f;
  float cg_bias_prior = 0.f;  // bias_value: -log((1 - PRIOR_PROB) / PRIOR_PROB), or the learned parameter with META_BIAS
  // ROIEncoder variant
  struct Lin { float* W = nullptr; float* b = nullptr; int K = 0, O = 0; };
  struct EncLayer { Lin attn, l1, l2; GNLayer n1, n2; };
  struct RoiEnc {
    ConvLayer pool_conv; GNLayer pool_gn;
    MsCamWeights cam;
    std::vector<ConvLayer> tok_conv; std::vector<GNLayer> tok_gn;
    std::vector<Lin> tok_fc, wh, bh;
    std::vector<EncLayer> layers;
  } re;
  bool has_backbone = false, has_head = false, has_codegen = false, has_roienc = false;
  // plans
  std::map<std::tuple<int, int, int>, std::unique_ptr<Plan>> plans;
  std::map<std::pair<int, int>, std::shared_ptr<struct PilCoeffs>> pil_cache;  // (in size, out size) -> resampling tables
  std::map<const void*, void*> hp_weights;  // conv_hpipe.hip re-packed copies of 3x3 weights, keyed by the igemm-layout pointer
  std::map<const void*, std::pair<void*, float*>> pw_weights;  // conv_pw.hip stage-image copies of 1x1 weights + scale/shift tables, keyed by the igemm-layout pointer
  void* pw_trash = nullptr;                 // conv_pw.hip trash slots (4 KiB)
  Plan* cur = nullptr;
  // Query records: `rec` is the record that is the current batch (nullptr: a fresh batch; then cur is the plan that scores it), `records`
  // every live record this context allocated
  const sylph_record* rec = nullptr;
  std::vector<sylph_record*> records;
  // sylph_merge_views, sylph_merge_views_large: the call's view tables (scratch: rewritten by every call; the event guards the host copy's reuse)
  void* merge_tab = nullptr;
  size_t merge_tab_cap = 0;
  std::vector<char> merge_host;
  hipEvent_t merge_ev = nullptr;
  // sylph_shot_combine: the call's index list and segment table (scratch like the merge tables: rewritten by every call, the event guards
  // the host copy's reuse) and, for the ROIEncoder, the class tokens and head activations of its segments
  void* shot_tab = nullptr;
  size_t shot_tab_cap = 0;
  std::vector<int> shot_host;
  hipEvent_t shot_ev = nullptr;
  float *shot_cls = nullptr, *shot_h = nullptr;
  int shot_seg_cap = 0;
  // sylph_cls_grad: the packed codes [32][256] and biases [32] of the class block in flight (stream order serialises the blocks of a call)
  void* ft_codes = nullptr;
  float* ft_bias = nullptr;
  // sylph_box_samples: the claiming box per row and the positives per 256-row block of the call in flight (scratch; grown on demand)
  int *bx_assign = nullptr, *bx_blk = nullptr;
  size_t bx_assign_cap = 0, bx_blk_cap = 0;
  // sylph_set_box_branch: 0 while pred / pred_taps / level_scales are the finalized tensors, else the value of the set that installed
  // them (box_stamp_next counts up); a query record keeps the stamp it was stored under
  uint64_t box_stamp = 0, box_stamp_next = 0;
  // the box branch as installed (box_w (Cout, 256, 3, 3) in torch order, box_b (Cout), level_scales) and as finalized (box_w0, box_b0, box_s0)
  std::vector<float> box_w, box_b, box_w0, box_b0, box_s0;
  // sylph_codegen_train_forward: the workspace and the episode sizes of the last forward (what a backward must be given again)
  void* cgt_ws = nullptr;
  int cgt_M = 0, cgt_nseg = 0, cgt_rows = 0;
  // sylph_set_code_generator: 0 while the support path runs the finalized generator, else the value of the set that installed the current
  // one (cg_stamp_next counts up); cg_flat / cg_flat0: the generator as installed / as finalized, in the flat layout of
  // sylph_codegen_param_layout (empty: the config is not trainable or no generator was loaded)
  uint64_t cg_stamp = 0, cg_stamp_next = 0;
  std::vector<float> cg_flat, cg_flat0;
  int* roi_rows_img = nullptr;  // sylph_roi_rows: the image table of the call in flight (grown on demand)
  size_t roi_rows_cap = 0;
  void* zeros = nullptr;  // 256 B of zeros (conv out-of-image taps)
  // small batches: the two FCOS towers of a head pass run on two streams (fork / join events around the bbox tower, api_head.hip)
  hipStream_t side_stream = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  int build_slot = 0;  // plan building: 1 while the ops being added will run on the side stream (split-K scratch slot, api_conv.hip)
  // optional per-launch timing of the MFMA conv kernel (bench.py roofline): HIP events on the launch stream
  bool prof = false;
  struct ProfRec { hipEvent_t a, b; double flops; const char* kern; };
  std::vector<ProfRec> prof_recs;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_free;
  std::vector<std::string> route_recs;  // while prof: one line per add_conv naming the ConvRoute it took (sylph_conv_routes_read)

  // Plan cache policy: every allocation made while a plan is being built / grown is owned by that plan, and
  // plans are evicted least-recently-used first once their count or their bytes exceed the budget, so a stream of
  // distinct padded shapes (real COCO / LVIS episodes) cannot grow HBM without bound.
  Plan* alloc_owner = nullptr;
  int64_t roi_table_uploads = 0;  // support calls that had to upload their ROI tables (sylph_roi_table_uploads)
  bool debug_taps = false;  // sylph_set_debug_taps: tower layers keep their outputs in separate buffers (parity tests)
  uint64_t use_clock = 0;
  size_t max_plans = 32;
  int64_t plan_byte_budget = 0;  // 0 = set from the device size at context creation
  int dalloc(void** p, size_t n);
  void dfree_nosync(void* p) {
    if (!p) return;
    for (size_t i = 0; i < allocs.size(); ++i)
      if (allocs[i] == p) { allocs[i] = allocs.back(); allocs.pop_back(); break; }
    auto it = alloc_bytes.find(p);
    if (it != alloc_bytes.end()) { bytes -= (int64_t)it->second; alloc_bytes.erase(it); }
    (void)hipFree(p);
  }
  std::map<void*, size_t> alloc_bytes;
  void dfree(void* p);  // release one dalloc'ed buffer (the stream may still use it: drained first)
  size_t esz() const { return dt == DT_BF16 ? 2 : 4; }
};

// One support pass of a plan (Plan::sup[R]): the workspaces, launches and parity taps of the code generator for S = R rows of 49
// positions.  Row r is the ROI (roi_image[r], boxes[r]) of the call's list; segments of consecutive rows are reduced to one code
// each.  One box per image (sylph_codegen, sylph_codegen_classes) is the list with roi_image[r] = r and equal segments.
struct SupportPass {
  int S = 0;           // rows: ROIs
  bool built = false;
  std::vector<OpFn> ops;
  void *roi = nullptr, *cgA = nullptr, *cgB = nullptr;
  float *cg_conv_out = nullptr, *cg_bias_out = nullptr, *cg_wnorm = nullptr;  // cg_wnorm: cls_weight_norm per class of the last call
  float *re_ctx = nullptr, *re_tok = nullptr, *re_tmp = nullptr, *re_hid = nullptr, *re_cls = nullptr, *re_h = nullptr;
  // support-path taps (sylph_export_support): (stage, index) -> where that stage's output of the last pass lives; the stages
  // whose buffer a later op overwrites are copied aside, only with debug taps on
  struct SupTap {
    const void* p = nullptr;
    bool f32 = true;  // fp32 buffer (else the context's storage type)
    int n = 0, npos = 49, C = 256, ld = 256;  // [n * npos][ld], first C channels (see api_codegen.hip tap_at)
    const float2* stats = nullptr;  // GroupNorm (mean, rstd) per (image, group) of the in-place apply, with its gamma / beta
    const float *gamma = nullptr, *beta = nullptr;
  };
  std::map<std::pair<int, int>, SupTap> taps;
  // sylph_codegen_shots: ops[0, n_shot_ops) are the per-shot stages (everything in front of the tail resp. the token mean);
  // shot_tok: the ROIEncoder's tokens after the last encoder layer, [S][256]
  size_t n_shot_ops = 0;
  const float* shot_tok = nullptr;
  // the current call (read by the ops at launch time)
  const float* cur_boxes = nullptr;
  int n_seg = 0;      // codes of the current call: the segments of its ROI list
  float* cur_code_out = nullptr;
  // the call's host tables as last uploaded (an unchanged list uploads nothing) and their device copies
  std::vector<int> roi_image, seg_len;
  int max_len = 0;             // longest segment of seg_len
  int* roi_image_dev = nullptr;  // [S]
  int2* seg_dev = nullptr;       // [S] capacity: {first row, rows} per segment
};

// What the last head entry left on a plan: all that sylph_decode_nms and sylph_export_head know about it.  Every head entry (and the export,
// where it writes missing logits) sets Plan::out to HeadOut() first and commits the whole record in ONE assignment as its last action: a
// failure in between leaves src none, answered with "sylph_fcos_head must be called first".  Nothing assigns single fields of Plan::out.
struct HeadOut {
  enum Src { none, cond, episodes, pretrained, imported, codesets } src = none;  // sylph_fcos_head | _episodes | _pretrained | sylph_import_head | sylph_fcos_head_codesets
  // Whose candidates logits_scan_kernel has already left in the decode buffers:
  //   cand_none     nobody's: the decode scans every image, after clearing the counters if Plan::cand_dirty says that an earlier fused
  //                 scan's candidates are still counted (a decode that ran its own scan leaves them zero: nms_kernel)
  //   cand_all      every image's (many-way sylph_fcos_head; the scan launch clears the counters itself): the decode skips its scan
  //   cand_scanned  those of the images whose episode takes the fused scan (mixed head; DecodeSeg::ncls < 0 in Plan::ep.dsegs):
  //                 decode_scan_kernel skips these images
  // In the last two nms_kernel keeps the counters, so a repeated decode finds the candidates again and the counters stay dirty.  A steady
  // stream of steps of one kind never clears in the decode (no extra launch).
  enum Cand { cand_none, cand_all, cand_scanned } cand = cand_none;
  bool has_bias = false;        // the class-conditional conv adds biases
  bool logits_missing = false;  // the logits columns of the scanned images were never written: sylph_export_head runs the unfused conv first
  int ncls = 0, logits_ld = 0;  // classes (of the widest episode / code set) and row pitch of Plan::logits
  int nsets = 0;                // codesets: G, the sets whose logits columns Plan::logits holds side by side (Plan::cs.col0)
};

// The packed class codes of one head call and their biases, in device buffers that grow with the request (api_head.hip: ensure_codes,
// upload_codes).  The uniform head, the episodes of a mixed head and the sets of a code-sets head each own one and read it the same way
// (cond_ep): codes and biases of a launch start at its first packed row.
struct PackedCodes {
  void* w = nullptr;       // [rows][row bytes]: [256] in the compute dtype; the 3x3 codes [3][3][256] (pack_conv's layout)
  float* bias = nullptr;   // [2][cap]: zero-padded biases | at bias + cap the same with -inf in the padding rows (logits_scan_kernel)
  int* src_row = nullptr;  // [rows]: row of the caller's (sum N, 256) table, -1 for a padding row (launch_pack_codes_episodes);
                           // nullptr: one N-way table, padded by launch_pack_codes / launch_pack_codes3x3
  int rows = 0, cap = 0;   // packed rows of the last call; capacity of the three buffers
};

// The decode buffers of `slots_cap` output slots with candidate buffers of `cand_cap` entries per (slot, level) (api_head.hip:
// ensure_decode_slots)
struct DecodeSlots {
  DecodeBuffers buf{};
  int slots_cap = 0, cand_cap = 0;
};

struct Plan {
  std::vector<void*> allocs;  // device buffers owned by this plan (freed on eviction)
  int64_t bytes = 0;
  uint64_t last_use = 0;
  int B = 0, H = 0, W = 0;
  int hl[8], wl[8], off[8], Ltot = 0;
  std::vector<int> img_h, img_w;
  // backbone
  void *x0 = nullptr, *stem_out = nullptr, *pool_out = nullptr;
  void* F = nullptr;  // pyramid [B*Ltot][256]
  void* bk_trash = nullptr;  // trash slots of the fused bottleneck kernels
  // split-K partial planes (api_conv.hip): ONE fp32 scratch per stream slot (0 = the context's stream, 1 = its side stream), sized to
  // the largest split layer of the plan and reused by every split layer of that stream -- stream order serialises conv -> finish ->
  // next conv.  The ops read the pointer through the slot at launch time (the buffer may grow while the plan is still being built).
  float* splitk_scratch[2] = {nullptr, nullptr};
  size_t splitk_bytes[2] = {0, 0};
  // parity taps (sylph_export_stage / sylph_export_tower): where the stage outputs res2..res5 and, with debug taps on, every
  // tower layer's stored conv output and GroupNorm coefficient table live
  const void* stage_out[4] = {nullptr, nullptr, nullptr, nullptr};
  // res2 when its last block took the stride-2-output launch (build_backbone): stage_out[0] is then filled on demand -- the tap runs
  // tail_dense_ops, the dense launch of that block from its intact input into tail_dense (allocated on first use)
  bool tail_even = false;
  const void* tail_x = nullptr;  // the last block's input: the stage's other ping-pong buffer
  void* tail_dense = nullptr;
  std::vector<OpFn> tail_dense_ops;
  int stage_h[4] = {0, 0, 0, 0}, stage_w[4] = {0, 0, 0, 0}, stage_c[4] = {0, 0, 0, 0};
  int stage_ld[4] = {0, 0, 0, 0};  // row pitch of stage_out where it is not stage_c (MobileNetV2: padded channels); 0 = stage_c
  std::vector<const void*> tap_out[2];      // [cls | bbox][layer]: conv output [rows][256] (pre-GroupNorm when tap_coef is set)
  std::vector<const float2*> tap_coef[2];   // [cls | bbox][layer]: (a, b) per (segment, channel), nullptr if applied in place
  std::vector<OpFn> backbone_ops, head_ops;
  bool backbone_built = false, head_built = false;
  ImageDesc* img_desc_dev = nullptr;
  ImageDesc* img_desc_host = nullptr;
  std::vector<ImageDesc> img_desc_last;  // what img_desc_dev holds (sylph_preprocess skips the H2D copy of an unchanged table)
  int img_desc_kind = 0;                 // 1: img_desc_dev was written by sylph_preprocess; anything else invalidates the cache
  hipEvent_t img_desc_ev = nullptr;  // recorded after the H2D copy of img_desc_host / rz_host (guards their reuse)
  // fused resize input pipeline: per-image descriptors + PIL coefficient tables (pinned host staging, device copy)
  ResizeDesc* rz_desc_dev = nullptr;
  char* rz_host = nullptr;  // [B descs][int table]
  int* rz_tab_dev = nullptr;
  size_t rz_tab_cap = 0;
  // head
  void *tA = nullptr, *tB = nullptr, *tC = nullptr, *tD = nullptr;
  void* cls_feat = nullptr;  // output of the cls tower (input of the class-conditional conv)
  // bf16: the last cls-tower GroupNorm is NOT applied by the head ops; sylph_fcos_head either fuses it into the
  // class-conditional conv (N <= 32: head_fused.hip) or runs cls_apply first
  const float2* cls_coef = nullptr;
  std::function<int(hipStream_t)> cls_apply;
  GnDeferred cls_gn;        // cls_coef with its size and the partials cls_apply reads (a query record keeps both)
  // State of the towers' outputs in this plan's buffers, for sylph_record_store: the head ops ran on the current fresh batch and nothing
  // has overwritten cls_feat / pred since; the deferred last cls GroupNorm has been applied in place since they ran
  bool towers_fresh = false, cls_applied = false;
  TowerSrc src;             // set by every head entry (run_towers): read by its launches, by sylph_export_head and by the decodes
  float* pred = nullptr;    // [rows][8]
  float* logits = nullptr;  // [rows][out.logits_ld], capacity [rows][logits_cap_ld]
  int logits_cap_ld = 0;
  HeadOut out;              // what the last head entry left in logits / pred / the decode buffers
  PackedCodes codes;        // the last sylph_fcos_head's 1x1 codes [Npad][256] and biases (Npad: cond_pad)
  void* code_wf = nullptr;  // workspace of logits_scan_kernel: the codes of one scan in MFMA fragment order; grows with the logits' class count
  int code_wf_cap = 0;
  // 3x3 class codes (cg_code_ksize 3): packed [Npad][3][3][256] with their biases and, per (N, bias or not), the conv launch add_conv
  // built on them -- valid while the buffers it captured are the plan's (cond3_for)
  PackedCodes codes3;
  std::map<std::pair<int, int>, std::vector<OpFn>> cond3_ops;
  const void* cond3_for[3] = {nullptr, nullptr, nullptr};  // codes3.w, logits, codes3.bias the ops read
  const SegDesc* head_segs = nullptr;
  const int2 *head_tiles = nullptr, *head_tiles32 = nullptr;
  int head_mtiles = 0, head_BM = 128, head_mtiles32 = 0;
  RowSeg* head_rowsegs = nullptr;
  float* gn_partial = nullptr;
  float2* gn_stats = nullptr;
  // decode
  DecodeSeg* dsegs = nullptr;
  // B slots (sylph_decode_nms) and G * B slots (sylph_decode_nms_codesets): two instances, so neither kind of step reallocates when the
  // two alternate
  DecodeSlots dec, dec_cs;
  bool cand_dirty = false;  // the candidate counters of dec are not zero: a fused scan filled them (a fact about the buffers: it survives heads)
  bool decode_built = false;
  std::vector<OpFn> cls_logits_ops;  // the checkpoint's cls_logits conv on this plan's cls tower output (sylph_fcos_head_pretrained)
  const float* cls_logits_dst = nullptr;  // the logits buffer those ops were built for
  int pool_cap = 0;
  bool stem_takes_raw = false;  // this plan's first backbone op is the fused stem + pool kernel (bf16): it can read raw images
  bool raw_input = false;     // the batch came in through sylph_preprocess and its normalisation is fused into the stem kernel
                              // (launch_stem_pool_raw reads the caller's images through img_desc_dev): x0 has NOT been written
  // Mixed-episode head (sylph_fcos_head_episodes): image i was run with the codes of episode ep.image[i].  The tables are read only
  // while out.src says that the plan's head outputs are such a head's.
  struct Episodes {
    PackedCodes codes;                   // every episode's rows, padded per episode as in sylph_fcos_head
    std::vector<int> n, image;           // classes per episode, episode per image: what the device tables below were built for
    std::vector<int> row0;               // per episode: its first row in `codes`
    std::vector<int2> tiles32, tilesBM;  // per episode: {first, count} of its tiles in tiles_dev (128-row tiles | head_BM-row tiles)
    int* seg_row0 = nullptr;             // [B * levels]: first packed row of the segment's episode
    int2* tiles_dev = nullptr;           // the tiles of the head's two tile tables regrouped episode by episode
    DecodeSeg* dsegs = nullptr;          // the decode's segment table with DecodeSeg::ncls set per image
  } ep;
  // Code-sets head (sylph_fcos_head_codesets): every image is scored against G code sets; the logits of set g are columns
  // [cs.col0[g], cs.col0[g] + cs.n[g]) of Plan::logits, and packed code row r produces column r.  The sets that take the fused
  // GroupNorm + conv kernel (bf16, cls GroupNorm deferred, N <= 32: gn_logits_sets_kernel) come first, each at a multiple of 4 (the
  // decode scan reads 16 bytes at a time), in cs.hot_blocks blocks of 32 rows; every other set follows at a multiple of 32 with the
  // padded width conv_igemm gives it in sylph_fcos_head.  Read only while out.src says that the head outputs are such a head's.
  struct CodeSets {
    PackedCodes codes;  // every set's rows (the copy of the biases for a scan is written and never read)
    std::vector<int> n, col0;
    int hot_blocks = 0, hot_width = 0, ld = 0;
    DecodeSeg* dsegs = nullptr;  // [G][B][levels]: DecodeSeg::ncls, cls0 and slot per set
    int dsegs_cap = 0;
  } cs;
  ImageOut* img_out_dev = nullptr;
  ImageOut* img_out_host = nullptr;
  std::vector<ImageOut> img_out_last;  // what img_out_dev holds (the H2D copy is skipped when a call's scales equal it)
  hipEvent_t img_out_ev = nullptr;  // recorded after the H2D copy of img_out_host (guards its reuse without a stream sync)
  // support
  LevelDesc* lv_dev = nullptr;  // per (image, level) of the batch: B x nlevels entries, shared by every support pass of the plan
  // one support pass per row count R (workspaces and conv routes follow R as they follow B above); sylph_codegen[_classes] use R = B
  std::map<int, std::unique_ptr<SupportPass>> sup;
  SupportPass* sup_last = nullptr;  // the pass of the last code-generator call on this plan (taps, cls_weight_norm)
};

// allocations made inside the scope belong to plan P (nullptr: to the context, e.g. re-packed weights)
struct OwnerScope {
  sylph_ctx* c; Plan* prev;
  OwnerScope(sylph_ctx* c_, Plan* P) : c(c_), prev(c_->alloc_owner) { c->alloc_owner = P; }
  ~OwnerScope() { c->alloc_owner = prev; }
};
// an allocation the context owns whichever plan is being built: plan eviction never frees it
inline int ctx_alloc(sylph_ctx* c, void** p, size_t n) {
  OwnerScope own(c, nullptr);
  return c->dalloc(p, n);
}

struct Geom {
  const SegDesc* segs;
  const int2* tiles;
  int n_mtiles;
  std::vector<int2> seg_tiles;  // per segment: {first tile, tile count}
  float* gn_partial = nullptr;  // per-tile GroupNorm partials written by the conv epilogue (want_gn)
};

struct ConvOpts {
  int stride = 1, pad = 0;
  int relu_nch = 0, mul_nch = 0;
  const void* res = nullptr;
  int res_ld = 0, res_mode = 0;
  bool out_f32 = false;
  int cout_override = -1;  // logical Cout (class-conditional conv)
  int stem = 0;            // ResNet stem loader
  int want_gn = 0;         // leave per-tile GroupNorm partials in the epilogue
  const void* in2 = nullptr;  // dual-source pointwise conv: second input, its row stride / channels / stride
  int in2_ld = 0, Cin2 = 0, stride2 = 1;
  double flops = -1.0;     // algorithmic FLOPs of the launch when they differ from 2*M*N*K (stem padding)
  const float2* gn_coef = nullptr;  // fused GroupNorm(+ReLU) of the INPUT (conv_hpipe.hip): (a, b) per (segment, input channel)
  int gn_relu = 0;
  int segs_per_image = 1;  // consecutive segments that belong to one image (pyramid-wide launches: the FPN levels)
  int stream_slot = 0;     // 1: the op will run on the context's side stream (its split-K scratch must not be the main stream's)
  int route_stride = 0;    // != 0: pick_conv_route decides as if `stride` were this (a strided 1x1 whose input was already subsampled by
                           // its producer keeps the launch of the strided layer: same kernel, same tiles, same K order)
};

// The kernel add_conv launches for one conv (pick_conv_route), with its tiles, LDS stages and K split:
//   hpipe         conv_hpipe.hip: 256 x 256 tiles over PAIRS of 3x3 halo patches, weights re-packed into stage images
//   igemm_halo    conv_igemm.hip on 128-position halo patches (3x3 s1 p1)
//   pw, spw       conv_pw.hip / conv_spw.hip: persistent pointwise kernels (conv_pw weight table, one PwDesc per M tile)
//   igemm_splitk  conv_igemm.hip split along K into fp32 partial planes + splitk_finish_kernel
//   igemm         conv_igemm.hip on BM-row tiles
enum class ConvKind { hpipe, igemm_halo, pw, spw, igemm_splitk, igemm };
struct ConvRoute {
  ConvKind kind = ConvKind::igemm;
  int BM = 0, BN = 0;
  int nbuf = 0;    // conv_igemm LDS stages of the 64-row tiles of small launches (ConvArgs::nbuf2): 0 = one, 2, 3
  int ksplit = 1;  // igemm_splitk: K ranges
};

// The kernel of ONE dense 3x3 pad-1 conv + FrozenBN [+ residual] [+ ReLU] on whole images (pick_conv3_route):
//   rw3      conv_rw3.hip: 128 -> 128, weights in registers, ph x pw patches (FrozenBN + ReLU only: no residual input)
//   rw64     conv_rw64.hip: 64 -> 64, weights in registers, ph x pw patches
//   generic  add_conv: pick_conv_route decides
// The dedicated kernels push no route record (sylph_conv_routes_read lists add_conv's choices only).
enum class Conv3Kind { rw3, rw64, generic };
struct Conv3Route {
  Conv3Kind kind = Conv3Kind::generic;
  int ph = 0, pw = 0;
};

// How add_bottleneck builds one bottleneck block (pick_block_route):
//   fused_id       bottleneck.hip, ONE kernel: the res2 identity blocks (C 256, mid 64, stride 1), bf16
//   fused_id_even  the same kernel's stride-2-output launch (BK_EVEN_OUT)
//   fused_proj     bottleneck.hip, ONE kernel: the first res2 block (64 -> 64 -> 64 -> 256, projection folded into conv3's GEMM)
//   chain          conv1 (add_conv) -> conv2 (grouped: conv_group.hip | rw3: conv_rw3.hip | generic: add_conv) -> conv3 + shortcut (add_conv;
//                  fused_sc: both as one GEMM over K = [t2 | X])
enum class BlockForm { fused_id, fused_id_even, fused_proj, chain };
enum class Conv2Form { grouped, rw3, generic };
struct BlockRoute {
  std::string refuse;  // not empty: the block cannot be built as asked; the text add_bottleneck fails with
  int chunk = 0;       // images per build: B, or less for a ResNeXt block whose tensors would pass 2^31 elements -- such a block is built
                       // chunk by chunk, every chunk with a pick of its own, and the fields below are not set
  BlockForm form = BlockForm::chain;
  Conv2Form conv2 = Conv2Form::generic;
  int ph = 0, pw = 0;     // conv2 == rw3: its patch
  bool fused_sc = false;  // chain: conv3 and the projection shortcut are one GEMM
  bool tail_ok = false;   // the block can take BK_EVEN_OUT: a fused identity block on a map of even height and width
  int s1 = 1, s3 = 1, H1 = 0, W1 = 0, Ho = 0, Wo = 0;  // strides of conv1 / conv2, conv1's output map, the block's output map
  // chain form, bf16, both blocks identity blocks 512 -> 128 -> 512 at stride 1 (R-50 / R-101 res3 blocks 1 .. n - 1):
  bool pair_ok = false;   // this block and `next` can run as a pair: conv3 + residual of this one also leaves next's conv1 output in t1
  bool pair_out = false;  // BK_PAIR_OUT was asked and granted: conv3 is the pair launch (conv_spw_pair.hip)
  bool pair_in = false;   // BK_PAIR_IN: conv1 is not built, t1 holds its output already
};

// How add_mbv2_block builds one InvertedResidual block (pick_mbv2_route): chain = expand (add_conv) -> dwconv3x3 -> project (add_conv);
// fused = ONE conv_mbv2 launch, bf16
enum class Mbv2Route { chain, fused };

// The stem + max-pool launches of build_backbone (pick_stem_route): stem_pool_kernel | stem_conv_kernel + maxpool | add_conv's stem loader + maxpool
enum class StemRoute { fused_pool, stem_conv, igemm };

struct BkScratch { void *t1, *t2, *sc; void** trash; };
// add_bottleneck flags
//   BK_EVEN_OUT    the block's output only at even rows / columns, Y compact [B][Hin/2 * Win/2][cout]: the fused identity block of
//                  res2 alone (bottleneck.hip, EVEN); anything else is refused
//   BK_IN_COMPACT  X is the compact output of such a block and Hin x Win its size: the (first, stride-2, stride-in-1x1) block is
//                  passed stride 1 and runs the strided block's launches on the rows it would have picked
//   BK_PAIR_OUT    conv3 + residual of this block and conv1 of `next` as one launch that leaves next's conv1 output in scr.t1 (the stage's
//                  t1 is free by then: this block's conv2 has read it); refused unless BlockRoute::pair_ok
//   BK_PAIR_IN     the block before was built with BK_PAIR_OUT: scr.t1 holds this block's conv1 output, the block starts at conv2
enum { BK_EVEN_OUT = 1, BK_IN_COMPACT = 2, BK_PAIR_OUT = 4, BK_PAIR_IN = 8 };

namespace sylph_host {
std::shared_ptr<PilCoeffs> pil_bilinear_coeffs(int in_size, int out_size);
// api_core.hip
void free_plan(sylph_ctx* c, Plan* P);
int upload(sylph_ctx* c, void** dev, const void* host, size_t n);
void evict_plans(sylph_ctx* c, const Plan* keep);
void drop_plan(sylph_ctx* c, Plan* P);
Plan* get_plan(sylph_ctx* c, int B, int H, int W);
int run_ops(sylph_ctx* c, const std::vector<OpFn>& ops, const char* what);
// The context's side stream: a second chain of small launches runs on it between a fork and a join (the FPN's top levels in
// build_backbone, the bbox tower in build_head).  The builder collects that chain's ops in a list of its own and appends them, each
// through on_side_stream, in front of the join op.  A split-K conv of the chain takes the side stream's scratch (ConvOpts::stream_slot
// or sylph_ctx::build_slot).
int ensure_side_stream(sylph_ctx* c);  // the stream and its two events, created on first use
OpFn side_fork_op(sylph_ctx* c);       // the side stream continues from here (fails with -101)
OpFn side_join_op(sylph_ctx* c);       // the op's stream waits for what the side stream was given (fails with -102)
OpFn on_side_stream(sylph_ctx* c, const OpFn& op);  // `op`, launched on the side stream whatever stream the op list runs on
// api_weights.hip
const HostTensor* find_w(sylph_ctx* c, const std::string& k);
int pack_conv(sylph_ctx* c, const std::vector<const HostTensor*>& ws, ConvLayer* L);
// a 256-input 3x3 conv in torch order, w (cout, 256, 3, 3): pack_conv's bf16 operand [cout_pad][tap][ci] (the rows past cout zero) ...
std::vector<uint16_t> pack_conv3x3_bf16(const float* w, int cout, int cout_pad);
// ... and the tap table of the fused GroupNorm + prediction pass, [64][256] bf16: row kh * sw + kw * cout + n, sw = roundup4(3 cout)
std::vector<uint16_t> pack_pred_taps(const float* w, int cout);
int upload_vec(sylph_ctx* c, float** dev, const std::vector<float>& v, int pad_to);
int make_conv_bn(sylph_ctx* c, const std::string& name, ConvLayer* L);
int pack_conv_grouped(sylph_ctx* c, const HostTensor& w, const std::string& key, int C, int groups, const float* scale, const float* shift,
                      ConvLayer* L);
int make_conv_bias(sylph_ctx* c, const std::vector<std::string>& names, ConvLayer* L);
int make_c3sc(sylph_ctx* c, const HostTensor& w3, const float* s3, const float* h3, const HostTensor& ws, const float* ss, const float* hs, ConvLayer* L);
int make_gn(sylph_ctx* c, const std::string& name, GNLayer* G);
void capture_code_generator(sylph_ctx* c);  // api_codegen_train.hip
int upload_f32(sylph_ctx* c, const float** dev, const HostTensor* t, const std::string& what, size_t expect = 0);
int make_lin(sylph_ctx* c, const std::string& name, sylph_ctx::Lin* L);
// a MobileNetV2 block from host tensors: w / scale / shift [3] = expand (nullptr for t == 1), depthwise (hid, 1, 3, 3), project
int make_mbv2_block(sylph_ctx* c, int cin, int t, int cout, int stride, const HostTensor* const* w, const float* const* scale, const float* const* shift,
                    sylph_ctx::MbBlock* blk);
int make_dw_table(sylph_ctx* c, const HostTensor& w, int C, int Cp, const float* scale, const float* shift, float** w_dev, float** scale_dev, float** shift_dev);
int make_ln(sylph_ctx* c, const std::string& name, GNLayer* G);
bool has_prefix(sylph_ctx* c, const std::string& p);
// api_conv.hip
void level_dims(const sylph_config& cfg, int H, int W, int* hl, int* wl, int* off, int* Ltot);
int make_geom(sylph_ctx* c, const std::vector<SegDesc>& segs, int BM, Geom* g);
void pick_patch(int H, int W, int max_pos, int halo_rows, int xpad, int* ph_out, int* pw_out);
void set_patch(SegDesc* s, int ph, int pw, int xpad);
int make_geom_patch(sylph_ctx* c, std::vector<SegDesc> segs, int max_pos, int halo_rows, int xpad, bool pair, Geom* g, int group = 1);
long patch_count(const std::vector<SegDesc>& segs, int max_pos, int halo_rows, int xpad);
int timed_op(sylph_ctx* c, const char* kern, double flops, hipStream_t s, const std::function<int(hipStream_t)>& fn);
ConvRoute pick_conv_route(const sylph_ctx* c, const ConvLayer& L, int in_ld, const std::vector<SegDesc>& segs, const ConvOpts& o);  // pure: no allocation, no upload
std::string conv_route_name(const ConvRoute& r);  // "igemm_splitk 64x64 nbuf2 ks8", "hpipe 256x256", "pw 128x256", ...
void adopt_records(sylph_ctx* c, sylph_ctx* tmp);  // parity entries: move a scratch context's profile + route records to the caller's
int add_conv(sylph_ctx* c, std::vector<OpFn>& ops, const ConvLayer& L, const void* in, int in_ld, void* out, int out_ld, const std::vector<SegDesc>& segs, const ConvOpts& o, Geom* geom_out = nullptr);
int add_conv_gn(sylph_ctx* c, std::vector<OpFn>& ops, const ConvLayer& L, const void* in, int in_ld, void* out, const std::vector<SegDesc>& segs, ConvOpts o, const GNLayer& G, int relu, const float2** coef_out = nullptr, OpFn* apply_out = nullptr, GnDeferred* deferred_out = nullptr);
int add_gn_from_partials(sylph_ctx* c, std::vector<OpFn>& ops, void* out, int ld, const std::vector<SegDesc>& segs, const Geom& g, const GNLayer& G, int relu,
                         const float2** coef_out, OpFn* apply_out, const float2** stats_out = nullptr, GnDeferred* deferred_out = nullptr);
int add_conv_deform(sylph_ctx* c, std::vector<OpFn>& ops, const ConvLayer& off, const ConvLayer& L, const void* in, void* out,
                    const std::vector<SegDesc>& segs, int segs_per_image, const GNLayer* G, int relu, const float2** coef_out = nullptr,
                    OpFn* apply_out = nullptr, GnDeferred* deferred_out = nullptr);
std::vector<SegDesc> image_segs(int B, int Hin, int Win, int Hout, int Wout, int resH = 0, int resW = 0);
// api_backbone.hip
int ensure_pyramid(sylph_ctx* c, Plan* P);
// the block-level pickers: pure (no allocation, no upload, no HIP call)
Conv3Route pick_conv3_route(const sylph_ctx* c, const ConvLayer& L, int B, int H, int W, int stride);
BlockRoute pick_block_route(const sylph_ctx* c, const sylph_ctx::Block& blk, int B, int Cin, int Hin, int Win, int stride, int mid, int cout, int flags,
                            const sylph_ctx::Block* next = nullptr);
StemRoute pick_stem_route(const sylph_ctx* c);
int add_bottleneck(sylph_ctx* c, std::vector<OpFn>& ops, const sylph_ctx::Block& blk, int B, const void* X, int Cin, int Hin, int Win, int stride, int mid, int cout, void* Y, const BkScratch& scr, int flags = 0,
                   const sylph_ctx::Block* next = nullptr);
// the pair launch alone (add_bottleneck with BK_PAIR_OUT; the parity entry sylph_res3_pair): dense t2 [B][HW][128], x / y [B][HW][512], t1 [B][HW][128]
int add_res3_pair(sylph_ctx* c, std::vector<OpFn>& ops, const ConvLayer& c3, const ConvLayer& c1_next, int B, int HW, const void* t2, const void* x, void* y, void* t1);
int add_conv3x3_c64(sylph_ctx* c, std::vector<OpFn>& ops, const ConvLayer& L, int B, int H, int W, const void* x, const void* res, void* y, int relu);
int add_basic_block(sylph_ctx* c, std::vector<OpFn>& ops, const sylph_ctx::Block& blk, int B, const void* X, int Cin, int Hin, int Win, int stride, int cout, void* Y, const BkScratch& scr);
// MobileNetV2 (cfg.mobilenet): channels as stored -- C rounded up to the K slice of the implicit-GEMM kernels (64 bf16, 32 fp32 modes)
inline int mbv2_pad(const sylph_ctx* c, int C) { const int q = c->dt == DT_BF16 ? 64 : 32; return (C + q - 1) / q * q; }
// ... and the row pitch of such a tensor: the Cout_pad pack_conv gives a layer of mbv2_pad(C) outputs.  conv_igemm launches Cout_pad / BN
// N tiles and its bf16 epilogue stores whole tiles whenever Cout % BN == 0, so a conv output needs rows of Cout_pad elements; the
// channels between mbv2_pad(C) and the pitch are never read.
inline int mbv2_ld(const sylph_ctx* c, int C) { const int p = mbv2_pad(c, C), q = p >= 128 ? 128 : (p > 32 ? 64 : 32); return (p + q - 1) / q * q; }
// One InvertedResidual block appended to `ops`: X [B][Hin * Win][cin_ld] -> Y [B][Ho * Wo][cout_ld]; h1 (the expand output, B * Hin * Win *
// hid_ld elements; unused when t == 1) and h2 (the depthwise output, B * Ho * Wo * hid_ld) are scratch.  Shared by build_backbone and
// the parity entry sylph_mbv2_block.
Mbv2Route pick_mbv2_route(const sylph_ctx* c, const sylph_ctx::MbBlock& blk, int B, int Hin, int Win);
// images per run when add_mbv2_block builds the chain (B unless a tensor of the block would pass 2^31 - 1 elements); fails by name for an
// image that is too large alone
int mbv2_chain_run(const sylph_ctx::MbBlock& blk, int B, int Hin, int Win, int* run);
int add_mbv2_block(sylph_ctx* c, std::vector<OpFn>& ops, const sylph_ctx::MbBlock& blk, int B, const void* X, int Hin, int Win, void* Y, void* h1, void* h2);
int add_dwconv3x3(sylph_ctx* c, std::vector<OpFn>& ops, const float* w, const float* scale, const float* shift, int B, int C, int ld, int H, int W,
                  int stride, const void* x, void* y);
int build_backbone(sylph_ctx* c, Plan* P);
// api_head.hip
std::vector<SegDesc> pyramid_segs(sylph_ctx* c, Plan* P);
int add_gn(sylph_ctx* c, Plan* P, std::vector<OpFn>& ops, void* x, const RowSeg* segs_dev, int nseg, int max_rows, const GNLayer& G, int relu);
int ensure_gn_ws(sylph_ctx* c, Plan* P, int nseg, int max_rows);
int build_head(sylph_ctx* c, Plan* P);
// A fresh batch becomes current on plan P (sylph_preprocess*, sylph_import_pyramid, sylph_import_head): a loaded query record is left, and
// whatever the towers left in P's buffers belongs to an earlier batch
void begin_fresh_batch(sylph_ctx* c, Plan* P);
// fails, naming `entry`, when the current batch is a query record (the entries that need the pyramid or the backbone's tensors)
int refuse_on_record(const sylph_ctx* c, const char* entry);
// api_codegen.hip
int build_support(sylph_ctx* c, Plan* P, SupportPass* Q);
int build_support_roienc(sylph_ctx* c, Plan* P, SupportPass* Q);
}  // namespace sylph_host
using namespace sylph_host;
