// Host side of libsylph_hip.so, unit "head": FCOS towers, class-conditional conv, decode + NMS (sylph_fcos_head*, sylph_decode_nms, head import / export).  The view merges over its detections are unit "views".
// No torch types, no CPU compute fallback: every stage is a HIP kernel from this directory.
#include "api_internal.h"

namespace sylph_host {

std::vector<SegDesc> pyramid_segs(sylph_ctx* c, Plan* P) {
  std::vector<SegDesc> v;
  for (int b = 0; b < P->B; ++b)
    for (int l = 0; l < c->cfg.nlevels; ++l) {
      SegDesc s;
      memset(&s, 0, sizeof(s));
      s.in_row0 = s.out_row0 = s.res_row0 = b * P->Ltot + P->off[l];
      s.in_H = s.out_H = s.res_H = P->hl[l];
      s.in_W = s.out_W = s.res_W = P->wl[l];
      s.mul = c->cfg.use_scale ? c->level_scales[l] : 1.f;
      v.push_back(s);
    }
  return v;
}

int add_gn(sylph_ctx* c, Plan* P, std::vector<OpFn>& ops, void* x, const RowSeg* segs_dev, int nseg,
                  int max_rows, const GNLayer& G, int relu) {
  const DType dt = c->dt;
  float* partial = P->gn_partial;
  float2* stats = P->gn_stats;
  const float *ga = G.gamma, *be = G.beta;
  ops.push_back([=](hipStream_t s) {
    return launch_groupnorm(dt, x, segs_dev, nseg, max_rows, 256, ga, be, 1e-5f, relu, partial, stats, s);
  });
  return 0;
}

int ensure_gn_ws(sylph_ctx* c, Plan* P, int nseg, int max_rows) {
  if (P->gn_partial) return 0;
  const int max_chunks = (max_rows + GN_ROWS_PER_CHUNK - 1) / GN_ROWS_PER_CHUNK;
  RET(c->dalloc((void**)&P->gn_partial, (size_t)nseg * max_chunks * 32 * 3 * sizeof(float)));
  RET(c->dalloc((void**)&P->gn_stats, (size_t)nseg * 32 * sizeof(float2)));
  return 0;
}

int build_head(sylph_ctx* c, Plan* P) {
  if (P->head_built) return 0;
  if (!c->has_head) return fail("FCOS head weights were not loaded");
  c->build_slot = 0;  // (an earlier build that failed half-way may have left it set)
  RET(ensure_pyramid(c, P));
  const size_t e = c->esz();
  const size_t rows = (size_t)P->B * P->Ltot;
  const int L = c->cfg.nlevels, nseg = P->B * L;
  RET(c->dalloc(&P->tA, rows * 512 * e));  // tA/tB, tC/tD: the ping-pong buffers of the cls / bbox towers
  RET(c->dalloc(&P->tC, rows * 512 * e));
  P->tB = (char*)P->tA + rows * 256 * e;
  P->tD = (char*)P->tC + rows * 256 * e;
  RET(c->dalloc((void**)&P->pred, rows * 8 * sizeof(float)));
  std::vector<RowSeg> rs;
  for (int b = 0; b < P->B; ++b)
    for (int l = 0; l < L; ++l) rs.push_back(RowSeg{b * P->Ltot + P->off[l], P->hl[l] * P->wl[l]});
  RET(upload(c, (void**)&P->head_rowsegs, rs.data(), rs.size() * sizeof(RowSeg)));
  const int max_rows = P->hl[0] * P->wl[0];
  // the support plan of the same shape may already own a GN workspace sized for fewer segments
  if (P->gn_partial) { P->gn_partial = nullptr; P->gn_stats = nullptr; }
  RET(ensure_gn_ws(c, P, nseg > P->B ? nseg : P->B, max_rows));
  const std::vector<SegDesc> segs = pyramid_segs(c, P);
  auto& main_ops = P->head_ops;
  const bool tower_gn = c->cfg.tower_norm == 0;  // MODEL.FCOS.NORM "GN"; otherwise "none": conv + bias + ReLU layers
  const void* tower_in = P->F;                    // what the cls / bbox towers read: the pyramid, or the shared tower's output
  // doff: MODEL.FCOS.USE_DEFORMABLE -- the offset conv of the tower's deformable last layer (nullptr: a plain tower)
  auto tower = [&](std::vector<OpFn>& ops, int which, const std::vector<ConvLayer>& convs, const std::vector<GNLayer>& gns, void* b0, void* b1,
                   void** last, const float2** coef_last, OpFn* apply_last, const ConvLayer* doff) -> int {
    const bool defer_last = coef_last != nullptr;
    const void* in = tower_in;
    void* out = b0;
    if (!tower_gn) {  // no norm layer: the ReLU is the conv epilogue's
      for (size_t i = 0; i < convs.size(); ++i) {
        ConvOpts o; o.pad = 1; o.segs_per_image = c->cfg.nlevels; o.relu_nch = 1 << 30;
        if (doff && i + 1 == convs.size()) RET(add_conv_deform(c, ops, *doff, convs[i], in, out, segs, c->cfg.nlevels, nullptr, 1));
        else RET(add_conv(c, ops, convs[i], in, 256, out, 256, segs, o));
        if (which < 2) { P->tap_out[which].push_back(out); P->tap_coef[which].push_back(nullptr); }
        in = out;
        out = (out == b0) ? b1 : b0;
        if (c->debug_taps && i + 1 < convs.size()) RET(c->dalloc(&out, rows * 256 * e));
      }
      *last = const_cast<void*>(in);
      return 0;
    }
    // GroupNorm + ReLU of layers 0 .. n-2 are applied by the NEXT layer's conv to its input halo in LDS (conv_hpipe.hip):
    // no separate streaming pass over those tensors.  The last layer keeps its apply pass (its readers are the
    // prediction convs and the class-conditional 1x1 conv).
    // A deformable last layer (doff) reads its input twice, through the offset conv and through the gather of conv_deform.hip: layer
    // n - 2 keeps its own GroupNorm apply pass so that this input is materialised once.
    ConvOpts probe; probe.pad = 1;
    const bool fuse = knob::gn_fuse() && convs.size() > 1 && convs[0].Cin <= 512 && pick_conv_route(c, convs[1], 256, segs, probe).kind == ConvKind::hpipe;
    const float2* coef_prev = nullptr;
    for (size_t i = 0; i < convs.size(); ++i) {
      ConvOpts o; o.pad = 1; o.segs_per_image = c->cfg.nlevels;
      if (coef_prev) { o.gn_coef = coef_prev; o.gn_relu = 1; }
      const float2* coef = nullptr;
      const bool is_last = i + 1 == convs.size();
      const bool feeds_deform = doff && i + 2 == convs.size();
      const bool defer = (fuse && !is_last && !feeds_deform) || (is_last && defer_last);
      OpFn apply;
      GnDeferred* keep = (is_last && defer_last && which == 0) ? &P->cls_gn : nullptr;  // (what a query record stores of this layer)
      if (doff && is_last)
        RET(add_conv_deform(c, ops, *doff, convs[i], in, out, segs, c->cfg.nlevels, &gns[i], 1, defer ? &coef : nullptr, defer_last ? &apply : nullptr, keep));
      else
        RET(add_conv_gn(c, ops, convs[i], in, 256, out, segs, o, gns[i], 1, defer ? &coef : nullptr, (is_last && defer_last) ? &apply : nullptr, keep));
      if (is_last && defer_last) { *coef_last = coef; *apply_last = apply; }
      coef_prev = coef;
      if (which < 2) { P->tap_out[which].push_back(out); P->tap_coef[which].push_back(coef); }
      in = out;
      out = (out == b0) ? b1 : b0;
      if (c->debug_taps && !is_last) RET(c->dalloc(&out, rows * 256 * e));  // keep every layer's output (same kernels, other destination)
    }
    *last = const_cast<void*>(in);
    return 0;
  };
  void *cls_feat = nullptr, *box_feat = nullptr;
  const float2* box_coef = nullptr;
  OpFn box_apply;
  // the cls tower's last GroupNorm is left to sylph_fcos_head (fused into the class-conditional conv when N <= 32)
  P->cls_coef = nullptr; P->cls_apply = nullptr; P->cls_gn = GnDeferred();
  const bool defer = knob::fuse_gn_logits() && c->dt == DT_BF16 && tower_gn;
  OpFn cls_apply;
  if (!c->share_tower.empty()) {
    // MODEL.FCOS.NUM_SHARE_CONVS (fcos.py:397,626): a shared tower in front of both; its last norm is applied in place (two readers)
    void *s0 = nullptr, *s1 = nullptr, *share_out = nullptr;
    RET(c->dalloc(&s0, rows * 256 * e));
    RET(c->dalloc(&s1, rows * 256 * e));
    RET(tower(main_ops, 2, c->share_tower, c->share_gn, s0, s1, &share_out, nullptr, nullptr, nullptr));
    tower_in = share_out;
  }
  // Small batches (SylphPredictor and the reference's query loop run batch 1, meta_learn_evaluation.py:421-426, predictor.py:248-274):
  // a tower layer is a launch of a few hundred blocks whose K loop is latency-bound, and the two towers are independent chains of
  // four such launches -> the bbox tower (+ its prediction pass) runs on a second stream between a fork and a join event, the cls
  // tower stays on the caller's stream.  Large batches fill the chip for many rounds per launch: one stream (measured equal).
  const int two_on = knob::head_streams();
  // Round 6: up to 32 full-size images (was 8): the two towers' launches of one layer share the last partial round of blocks -- batch 12
  // 1 737 -> 1 806 img/s, batch 16 / 24 / 32 +1 %, 48 ... 192 equal (profiles/r6_small_batch.md)
  const bool two_streams = two_on == 2 || (two_on == 1 && rows <= (size_t)32 * 22400);
  if (two_streams) {
    RET(ensure_side_stream(c));
    main_ops.push_back(side_fork_op(c));
  }
  RET(tower(main_ops, 0, c->cls_tower, c->cls_gn, P->tA, P->tB, &cls_feat, (defer && !c->cls_tower.empty()) ? &P->cls_coef : nullptr, &cls_apply,
            c->cls_off.Cout ? &c->cls_off : nullptr));
  P->cls_apply = cls_apply;
  const bool box_defer = defer && c->pred_taps && !c->box_tower.empty();
  // two streams: the bbox tower + prediction pass go to the side stream.  A split-K conv among them (towers without GroupNorm, the
  // prediction conv) must take the side stream's partial-plane scratch, not the one the cls tower is using at the same time
  std::vector<OpFn> side_ops;
  std::vector<OpFn>& ops = two_streams ? side_ops : main_ops;
  c->build_slot = two_streams ? 1 : 0;
  RET(tower(ops, 1, c->box_tower, c->box_gn, P->tC, P->tD, &box_feat, box_defer ? &box_coef : nullptr, &box_apply,
            c->box_off.Cout ? &c->box_off : nullptr));
  Geom g32;  // 128-row pointwise tiles of the pyramid (class-conditional conv with N <= 32, fused GN + prediction pass)
  RET(make_geom(c, segs, 128, &g32));
  if (box_defer && box_coef) {
    // last bbox-tower GroupNorm + the 3x3 prediction convs: one streaming pass for the nine tap responses + a gather (head_fused.hip)
    const int cp = c->pred.Cout, sw = (3 * cp + 3) & ~3;
    float* taps_ws = nullptr;
    const size_t plane_rows = rows;
    RET(c->dalloc((void**)&taps_ws, (size_t)3 * rows * sw * sizeof(float)));
    const void *xin = box_feat, *wt = c->pred_taps;
    const float* bias = c->pred.shift;
    float* pout = P->pred;
    const SegDesc* sgd = g32.segs; const int2* tld = g32.tiles; const int ntl = g32.n_mtiles;
    const float2* bc = box_coef;
    const double fl = 2.0 * (double)rows * cp * 9.0 * 256.0;
    ops.push_back([=](hipStream_t s) {
      return timed_op(c, "gn_taps_kernel+tap_gather_kernel", fl, s, [=](hipStream_t st) { return launch_gn_pred_taps(xin, 256, bc, wt, cp, bias, 4, 4, taps_ws, plane_rows, pout, 8, sgd, tld, ntl, st); });
    });
  } else {
    ConvOpts op; op.pad = 1; op.segs_per_image = c->cfg.nlevels; op.relu_nch = 4; op.mul_nch = 4; op.out_f32 = true;
    RET(add_conv(c, ops, c->pred, box_feat, 256, P->pred, 8, segs, op));
  }
  c->build_slot = 0;
  if (two_streams) {
    for (const OpFn& op : side_ops) main_ops.push_back(on_side_stream(c, op));
    main_ops.push_back(side_join_op(c));
  }
  // geometry for the class-conditional 1x1 conv (weights arrive per call)
  {
    Geom g;
    int BM, BN;
    conv_pick_tile((int)rows, 128, 9, &BM, &BN);  // geometry for BN in {64,128}; BM from the 128-wide rule
    RET(make_geom(c, segs, BM, &g));
    P->head_segs = g.segs; P->head_tiles = g.tiles; P->head_mtiles = g.n_mtiles; P->head_BM = BM;
    P->head_tiles32 = g32.tiles; P->head_mtiles32 = g32.n_mtiles;
  }
  P->cls_feat = cls_feat;
  P->head_built = true;
  return 0;
}

// Per-(image, level) capacity of the decode candidate buffers.  The reference has no cap (boolean-mask indexing,
// fcos_outputs.py:960-990); here the scan compacts into a fixed buffer and overflow is reported.  Up to 262 144 slots the
// buffer holds EVERY (location, class) score of the largest level (5-way: 84 000, 20-way: 262 144 of 336 000), i.e. it cannot
// overflow for few-shot class counts; many-way episodes get 1/8 of the scores (LVIS 866-way: 1.8 M), at most 4 M
// (HBM is plentiful: 8 bytes per slot).
static int want_cand_cap(const sylph_ctx* c, const Plan* P, int ncls) {
  if (c->cfg.cand_cap > 0) return c->cfg.cand_cap;
  const long all = (long)P->hl[0] * P->wl[0] * (long)(ncls > 0 ? ncls : 1);
  long w = all <= 262144 ? all : (all / 8 > 262144 ? all / 8 : 262144);
  if (w < 4096) w = 4096;
  if (w > (1L << 22)) w = 1L << 22;
  return (int)w;
}

// the decode's segment table; img_ncls[b]: DecodeSeg::ncls of image b (nullptr: 0 everywhere, the plan's own table)
static std::vector<DecodeSeg> decode_segs(const sylph_ctx* c, const Plan* P, const int* img_ncls) {
  std::vector<DecodeSeg> ds;
  for (int b = 0; b < P->B; ++b) {
    unsigned lb = 0;
    for (int l = 0; l < c->cfg.nlevels; ++l) {
      DecodeSeg d;
      d.row0 = b * P->Ltot + P->off[l]; d.nloc = P->hl[l] * P->wl[l]; d.W = P->wl[l];
      d.stride = c->cfg.strides[l]; d.level = l; d.image = b; d.loc_base = lb; d.ncls = img_ncls ? img_ncls[b] : 0;
      d.cls0 = 0; d.slot = b;
      lb += (unsigned)d.nloc;
      ds.push_back(d);
    }
  }
  return ds;
}

static int build_decode(sylph_ctx* c, Plan* P) {
  if (P->decode_built) return 0;
  const int L = c->cfg.nlevels, B = P->B;
  const std::vector<DecodeSeg> ds = decode_segs(c, P, nullptr);
  RET(upload(c, (void**)&P->dsegs, ds.data(), ds.size() * sizeof(DecodeSeg)));
  int pool = 64;
  while (pool < L * c->cfg.pre_nms_topk) pool <<= 1;
  if (pool > 8192) return fail("levels * PRE_NMS_TOPK exceeds the 8192-entry on-chip sort capacity");
  P->pool_cap = pool;  // (the decode buffers themselves: ensure_decode_slots)
  RET(c->dalloc((void**)&P->img_out_dev, sizeof(ImageOut) * B));
  HIPCHK(hipHostMalloc((void**)&P->img_out_host, sizeof(ImageOut) * B));
  P->decode_built = true;
  return 0;
}

// If need > *cap: release *ptr and allocate need * bytes_per_unit bytes.  Freed first, and *ptr null and *cap 0 across the allocation: a
// failure leaves no capacity that lies.
template <class T>
static int grow_dev(sylph_ctx* c, T** ptr, int* cap, int need, size_t bytes_per_unit) {
  if (need <= *cap) return 0;
  c->dfree(*ptr);
  *ptr = nullptr; *cap = 0;
  RET(c->dalloc((void**)ptr, (size_t)need * bytes_per_unit));
  *cap = need;
  return 0;
}

// Decode buffers S for `slots` output slots (B: sylph_decode_nms on Plan::dec; G * B: sylph_decode_nms_codesets on Plan::dec_cs) with
// candidate buffers for ncls classes per (slot, level).  Two tiers: the per-slot members are allocated, and zeroed once (every decode
// leaves them zero again: nms_kernel), when `slots` grows; cand_key / cand_idx are reallocated alone when the candidate capacity grows.
// Growth must never discard candidates that a fused scan has left for the decode.  It does not: the slots of Plan::dec never grow after
// the first call (B belongs to the plan), launch_cond grows the candidate buffers BEFORE it launches the scan, and the decode that
// follows asks for the same ncls (HeadOut::ncls); no head leaves candidates in Plan::dec_cs.
static int ensure_decode_slots(sylph_ctx* c, Plan* P, DecodeSlots& S, int slots, int ncls) {
  BUILD(build_decode(c, P), P);
  const size_t L = c->cfg.nlevels, pool = P->pool_cap;
  DecodeBuffers& d = S.buf;
  if (slots > S.slots_cap) {
    const struct { void** p; size_t per_slot; bool zero; } per[] = {
        {(void**)&d.cand_count, L * 4, true},   {(void**)&d.sel_ws, L * SEL_WS * 4, true}, {(void**)&d.sel_tie, L * SEL_TIE * 8, false},
        {(void**)&d.pool_key, pool * 8, false}, {(void**)&d.pool_count, 4, true},          {(void**)&d.s_box, pool * 16, false},
        {(void**)&d.s_score, pool * 4, false},  {(void**)&d.s_cls, pool * 4, false},       {(void**)&d.s_level, pool * 4, false},
        {(void**)&d.s_loc, pool * 8, false},    {(void**)&d.s_ord, pool * 4, false}};
    for (const auto& m : per) { c->dfree(*m.p); *m.p = nullptr; }
    c->dfree(d.cand_key); c->dfree(d.cand_idx);
    d.cand_key = nullptr; d.cand_idx = nullptr;
    S.slots_cap = 0; S.cand_cap = 0;
    for (const auto& m : per) {
      RET(c->dalloc(m.p, (size_t)slots * m.per_slot));
      if (m.zero) HIPCHK(hipMemsetAsync(*m.p, 0, (size_t)slots * m.per_slot, c->stream));
    }
    if (!d.status) {
      RET(c->dalloc((void**)&d.status, 8));
      HIPCHK(hipMemsetAsync(d.status, 0, 8, c->stream));
    }
    S.slots_cap = slots;
  }
  const int cap = want_cand_cap(c, P, ncls);
  if (cap > S.cand_cap) {
    const size_t bytes = (size_t)S.slots_cap * L * cap * 4;
    c->dfree(d.cand_key); c->dfree(d.cand_idx);
    d.cand_key = nullptr; d.cand_idx = nullptr; S.cand_cap = 0;
    RET(c->dalloc((void**)&d.cand_key, bytes));
    RET(c->dalloc((void**)&d.cand_idx, bytes));
    S.cand_cap = cap;
  }
  return 0;
}

static DecodeCfg decode_cfg(const sylph_ctx* c, const Plan* P, const DecodeSlots& S, const HeadOut& o, int max_out) {
  DecodeCfg d;
  d.num_classes = o.ncls; d.logits_ld = o.logits_ld; d.pre_nms_thresh = c->cfg.pre_nms_thresh;
  d.pre_nms_topk = c->cfg.pre_nms_topk; d.nms_thresh = c->cfg.nms_thresh; d.post_nms_topk = c->cfg.post_nms_topk;
  d.thresh_with_ctr = c->cfg.thresh_with_ctr; d.quality_mode = c->cfg.quality_mode; d.cand_cap = S.cand_cap;
  d.pool_cap = P->pool_cap; d.nlevels = c->cfg.nlevels; d.max_out = max_out;
  return d;
}

// column tile of an N-way class-conditional conv and N padded to it: the rows of its packed codes and biases
struct CondPad { int bn, Npad; };
static CondPad cond_pad(int N) {
  const int bn = N >= 128 ? 128 : (N > 32 ? 64 : 32);
  return {bn, (N + bn - 1) / bn * bn};
}

// The kernel of an N-way class-conditional conv, for the uniform head and for every episode of a mixed one alike:
//   gn_logits          last cls GroupNorm + ReLU + conv in one HBM pass (head_fused.hip): bf16, up to 32 classes
//   scan               conv + score scan in one pass, the logits never reach HBM (detect.hip: logits_scan_kernel): bf16, many-way
//   igemm_after_apply  conv_igemm once the last cls GroupNorm, which the head ops left out, has been applied in place
//   igemm              conv_igemm (the head ops applied every GroupNorm: fp32 storage, FCOS.NORM "none", SYLPH_FUSE_GN_LOGITS=0)
// allow_scan = false: the kernel that writes the logits a scan left out (sylph_export_head)
enum class HeadKind { gn_logits, scan, igemm_after_apply, igemm, gn_cond3x3 };  // gn_cond3x3: 3x3 codes only (head_kind3x3)
static HeadKind head_kind(const sylph_ctx* c, const Plan* P, int N, bool allow_scan = true) {
  const int fuse_scan_on = knob::fuse_scan();
  if (c->dt != DT_BF16 || !P->cls_coef) return HeadKind::igemm;
  if (allow_scan && fuse_scan_on && (N > 32 || fuse_scan_on == 2) && N < 65536) return HeadKind::scan;
  return N <= 32 ? HeadKind::gn_logits : HeadKind::igemm_after_apply;
}

// the three buffers of pc for `rows` packed rows of row_bytes bytes (src_row only where the caller packs through such a table)
static int ensure_codes(sylph_ctx* c, PackedCodes& pc, int rows, size_t row_bytes, bool with_src_row) {
  if (rows > pc.cap) {
    int cw = pc.cap, cb = pc.cap, cs = pc.cap;
    pc.cap = 0;  // (one capacity for the three: it holds only once all of them have grown)
    RET(grow_dev(c, &pc.w, &cw, rows, row_bytes));
    RET(grow_dev(c, &pc.bias, &cb, rows, 2 * sizeof(float)));
    if (with_src_row) RET(grow_dev(c, &pc.src_row, &cs, rows, sizeof(int)));
    pc.cap = rows;
  }
  pc.rows = rows;
  return 0;
}

// pc for the packed-row -> source-row table of a mixed or code-sets head, uploaded
static int upload_codes(sylph_ctx* c, PackedCodes& pc, const std::vector<int>& src_row) {
  HIPCHK(hipStreamSynchronize(c->stream));  // the previous step may still be reading the tables (this one, and those the caller uploads next)
  RET(ensure_codes(c, pc, (int)src_row.size(), 256 * c->esz(), true));
  HIPCHK(hipMemcpy(pc.src_row, src_row.data(), src_row.size() * sizeof(int), hipMemcpyHostToDevice));
  return 0;
}

// logits of the current batch for N classes and the fused scan's workspace for as many (grown on demand; the previous buffers are
// released) -> o->ncls, o->logits_ld
static int ensure_logits(sylph_ctx* c, Plan* P, int N, bool allow_narrow, HeadOut* o) {
  const size_t rows = (size_t)P->B * P->Ltot;
  const int Npad = cond_pad(N).Npad;
  RET(grow_dev(c, &P->logits, &P->logits_cap_ld, Npad, rows * sizeof(float)));
  RET(grow_dev(c, &P->code_wf, &P->code_wf_cap, Npad, 256 * c->esz()));
  // row pitch of the logits: the padded class count, except for <= 8 classes on the fused GroupNorm + class-conditional conv path
  // (gn_logits_kernel stores any multiple of 4 columns): 8 floats per location instead of 32 -- the conv writes and the scan reads
  // a quarter of the bytes (a 5-way episode: 46 MB instead of 183 MB per 64 images)
  o->logits_ld = allow_narrow && N <= 8 && head_kind(c, P, N, false) == HeadKind::gn_logits ? 8 : Npad;
  o->ncls = N;
  return 0;
}

// the deferred last cls GroupNorm, applied in place, with a profile record of its own
static int apply_cls_gn(sylph_ctx* c, Plan* P) {
  const Plan* PP = P;
  P->cls_applied = true;
  KCHK(timed_op(c, "gn_apply_partials_kernel", 0.0, c->stream, [=](hipStream_t st) { return PP->cls_apply(st); }), "gn_apply (cls tower, last layer)");
  return 0;
}

// ---- the towers' outputs of the current batch: a fresh batch's in the plan's buffers, or a query record's ------------------------------

void begin_fresh_batch(sylph_ctx* c, Plan* P) {
  // the plan that scored the record may hold logits of it and sources that point into it: nothing of that describes a later batch
  if (c->rec && c->cur) c->cur->out = HeadOut();
  c->rec = nullptr;
  P->towers_fresh = false;
}

int refuse_on_record(const sylph_ctx* c, const char* entry) {
  if (!c->rec) return 0;
  return fail(std::string(entry) + ": the current batch is a query record (sylph_record_load), which holds the towers' outputs and no pyramid; "
              "make a fresh batch current first");
}

// The record's tower outputs, copied into the plan's own buffers: for the routes that normalise cls_feat in place or run conv launches built
// on the plan's pointers (fp32 storage, FCOS.NORM "none", igemm_after_apply, 3x3 codes, the pretrained head, the logits export after a
// scan).  With the partials the deferred apply reads, so that it runs exactly as on the fresh batch.  pred is never copied: nothing writes it.
static int restore_record(sylph_ctx* c, Plan* P) {
  const sylph_record* R = c->rec;
  HIPCHK(hipMemcpyAsync(P->cls_feat, R->feat, R->feat_bytes, hipMemcpyDeviceToDevice, c->stream));
  if (R->coef) {
    HIPCHK(hipMemcpyAsync(const_cast<float2*>(P->cls_gn.coef), R->coef, R->coef_bytes, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(const_cast<float*>(P->cls_gn.partial), R->partial, R->partial_bytes, hipMemcpyDeviceToDevice, c->stream));
  }
  P->src.feat = P->cls_feat; P->src.coef = P->cls_coef; P->src.pred = R->pred;
  return 0;
}

// What every head entry does where the class-agnostic part of the step belongs.  A fresh batch: the head ops (towers, box heads, cls
// GroupNorm statistics).  A query record: no launch at all when every kernel of the call streams its operands through pointers
// (`streaming`: gn_logits, the sets and episodes kernels, the fused scan) -- they read the record in place -- and restore_record otherwise.
static int run_towers(sylph_ctx* c, Plan* P, bool streaming) {
  if (c->rec) {
    if (!streaming) return restore_record(c, P);
    P->src.feat = c->rec->feat; P->src.coef = c->rec->coef; P->src.pred = c->rec->pred;
    return 0;
  }
  P->towers_fresh = false;
  RET(run_ops(c, P->head_ops, "fcos_head"));
  P->towers_fresh = true; P->cls_applied = false;
  P->src.feat = P->cls_feat; P->src.coef = P->cls_coef; P->src.pred = P->pred;
  return 0;
}

// ---- 3x3 class codes (CODE_GENERATOR.CLS_LAYER kernel size 3; sylph_fcos_head only) ---------------------------------------------------
// The kernel of an N-way 3x3 class-conditional conv (padding 1 on the normalised tower output):
//   gn_cond3x3         last cls GroupNorm + ReLU + 3x3 conv in one pass (head_fused.hip): bf16, up to 32 classes, only with SYLPH_GN_COND3X3=1 --
//                      measured 0.73 / 0.80 ms (N = 5 / 32, 64 images) against 0.63 / 0.61 ms for the two launches below, so not the default
//   igemm_after_apply  the deferred GroupNorm apply, then add_conv on the packed codes -- what sylph_fcos_head_pretrained builds for a 3x3
//   igemm              cls_logits, with weights that arrive per call (fp32 storage, FCOS.NORM "none", SYLPH_FUSE_GN_LOGITS=0: no apply left)
// The fused score scan never takes 3x3 codes.
static HeadKind head_kind3x3(const sylph_ctx* c, const Plan* P, int N) {
  if (c->dt != DT_BF16 || !P->cls_coef) return HeadKind::igemm;
  return (N <= 32 && knob::gn_cond3x3()) ? HeadKind::gn_cond3x3 : HeadKind::igemm_after_apply;
}

// the conv launch of the generic route for o.ncls classes, built once per (N, bias) on the plan's current buffers
static int cond3x3_conv_ops(sylph_ctx* c, Plan* P, const HeadOut& o, const std::vector<OpFn>** ops_out) {
  if (P->cond3_for[0] != P->codes3.w || P->cond3_for[1] != P->logits || P->cond3_for[2] != P->codes3.bias) {
    P->cond3_ops.clear();
    P->cond3_for[0] = P->codes3.w; P->cond3_for[1] = P->logits; P->cond3_for[2] = P->codes3.bias;
  }
  const std::pair<int, int> key(o.ncls, o.has_bias ? 1 : 0);
  auto it = P->cond3_ops.find(key);
  if (it == P->cond3_ops.end()) {
    ConvLayer L;
    L.w = P->codes3.w; L.shift = o.has_bias ? P->codes3.bias : nullptr;
    L.Cin = 256; L.Cout = o.ncls; L.Cout_pad = cond_pad(o.ncls).Npad; L.KH = 3; L.KW = 3;
    ConvOpts op; op.pad = 1; op.segs_per_image = c->cfg.nlevels; op.out_f32 = true;
    std::vector<OpFn> ops;
    RET(add_conv(c, ops, L, P->cls_feat, 256, P->logits, o.logits_ld, pyramid_segs(c, P), op));
    it = P->cond3_ops.emplace(key, std::move(ops)).first;
  }
  *ops_out = &it->second;
  return 0;
}

// sylph_fcos_head with cg_code_ksize 3, after the checks and build_head: cls_conv is (N, 256, 3, 3)
static int fcos_head_3x3(sylph_ctx* c, Plan* P, const float* cls_conv, const float* cls_bias, int N) {
  HeadOut o;
  o.src = HeadOut::cond;
  o.has_bias = c->cfg.cond_use_bias && cls_bias;
  const HeadKind k = head_kind3x3(c, P, N);
  // Deformable towers promise the default route's detections bit for bit from every entry (tests/test_head_variants_gpu.py).  The fused
  // kernel cannot give them: it adds nine per-tap fp32 accumulators in a fixed order, conv_igemm runs one accumulator over K = 2 304, and
  // a score comes out one fp32 ulp apart (3.6e-7 measured).  Refused before anything is launched, not run as a near miss.
  if (k == HeadKind::gn_cond3x3 && c->cfg.tower_deformable)
    return fail("SYLPH_GN_COND3X3=1 with MODEL.FCOS.USE_DEFORMABLE: gn_cond3x3_kernel sums its nine taps in another order than the default route "
                "(GroupNorm apply + conv_igemm) and its scores differ from that route's in the last fp32 bit; the fused 3x3 route is not offered "
                "for deformable towers (unset SYLPH_GN_COND3X3)");
  RET(ensure_logits(c, P, N, false, &o));
  const int Npad = cond_pad(N).Npad;
  if (k == HeadKind::gn_cond3x3 && N <= 8) o.logits_ld = 8;  // as gn_logits: the fused kernel stores any multiple of 4 columns
  PackedCodes& pc = P->codes3;
  RET(ensure_codes(c, pc, Npad, 9 * 256 * c->esz(), false));
  // one launch in front of the towers, as for the 1x1 codes
  KCHK(launch_pack_codes3x3(c->dt, cls_conv, N, 256, Npad, pc.w, o.has_bias ? cls_bias : nullptr, pc.bias, pc.bias + pc.cap, c->stream), "pack_codes3x3");
  RET(run_towers(c, P, false));
  if (k == HeadKind::gn_cond3x3) {
    const Plan* PP = P;
    const float* bias = o.has_bias ? pc.bias : nullptr;
    const int ld = o.logits_ld;
    KCHK(timed_op(c, "gn_cond3x3_kernel", 2.0 * (double)P->B * P->Ltot * N * 2304.0, c->stream, [=](hipStream_t st) {
           return launch_gn_cond3x3(PP->src.feat, 256, PP->src.coef, PP->codes3.w, bias, N, PP->logits, ld, PP->head_segs, PP->head_tiles32,
                                    PP->head_mtiles32, st);
         }), "gn_cond3x3");
  } else {
    if (k == HeadKind::igemm_after_apply) RET(apply_cls_gn(c, P));
    const std::vector<OpFn>* ops = nullptr;
    RET(cond3x3_conv_ops(c, P, o, &ops));
    RET(run_ops(c, *ops, "cond_cls_logits 3x3"));
  }
  o.cand = HeadOut::cand_none;
  P->out = o;
  return 0;
}

// ---- class-conditional conv: one launcher for the uniform head (sylph_fcos_head) and the episodes of a mixed one ------------------------

// Host and device tables of a mixed batch: packed-row layout of the episodes' codes, segment -> code rows, the head's tiles regrouped
// episode by episode, the decode's segment table with per-image class counts.  Rebuilt only when (n_classes, image_episode) differ
// from the previous call's on this plan: a serving loop that keeps its assignment uploads nothing.
static int ep_tables(sylph_ctx* c, Plan* P, int E, const int* n_classes, const int* image_episode) {
  const int L = c->cfg.nlevels, B = P->B, nseg = B * L;
  std::vector<int> en(n_classes, n_classes + E), ei(image_episode, image_episode + B);
  Plan::Episodes& T = P->ep;
  if (T.dsegs && en == T.n && ei == T.image) return 0;
  T.n.clear(); T.image.clear();  // (a failure below leaves no key that would match half-written tables)
  std::vector<int> row0(E), src_row;
  int src = 0;
  for (int e = 0; e < E; ++e) {
    const int N = en[e], npad = cond_pad(N).Npad;
    row0[e] = (int)src_row.size();
    for (int r = 0; r < npad; ++r) src_row.push_back(r < N ? src + r : -1);
    src += N;
  }
  std::vector<std::vector<int>> members(E);
  for (int b = 0; b < B; ++b) members[ei[b]].push_back(b);
  std::vector<int2> tiles, t32(E), tBM(E);
  for (int pass = 0; pass < 2; ++pass) {  // the tile order inside an image is make_geom's
    const int BM = pass == 0 ? 128 : P->head_BM;
    for (int e = 0; e < E; ++e) {
      const int first = (int)tiles.size();
      for (int b : members[e])
        for (int l = 0; l < L; ++l)
          for (int r = 0; r < P->hl[l] * P->wl[l]; r += BM) tiles.push_back(make_int2(b * L + l, r));
      (pass == 0 ? t32 : tBM)[e] = make_int2(first, (int)tiles.size() - first);
    }
  }
  if ((int)tiles.size() != P->head_mtiles32 + P->head_mtiles) return fail("internal: episode tile tables");
  std::vector<int> seg_row0(nseg), img_ncls(B);
  for (int b = 0; b < B; ++b) {
    const int N = en[ei[b]];
    for (int l = 0; l < L; ++l) seg_row0[b * L + l] = row0[ei[b]];
    img_ncls[b] = head_kind(c, P, N) == HeadKind::scan ? -N : N;  // negative: the fused scan leaves this image's candidates
  }
  const std::vector<DecodeSeg> ds = decode_segs(c, P, img_ncls.data());
  RET(upload_codes(c, T.codes, src_row));
  if (!T.seg_row0) RET(c->dalloc((void**)&T.seg_row0, (size_t)nseg * sizeof(int)));
  if (!T.tiles_dev) RET(c->dalloc((void**)&T.tiles_dev, tiles.size() * sizeof(int2)));
  if (!T.dsegs) RET(c->dalloc((void**)&T.dsegs, (size_t)nseg * sizeof(DecodeSeg)));
  HIPCHK(hipMemcpy(T.seg_row0, seg_row0.data(), (size_t)nseg * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(T.tiles_dev, tiles.data(), tiles.size() * sizeof(int2), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(T.dsegs, ds.data(), ds.size() * sizeof(DecodeSeg), hipMemcpyHostToDevice));
  T.row0 = row0; T.tiles32 = t32; T.tilesBM = tBM;
  T.n = en; T.image = ei;
  return 0;
}

// Inputs of one class-conditional conv launch: the N-way codes wt [cond_pad(N).Npad][256], their biases (nullptr: none) and the copy with
// -inf in the padding rows that the fused scan reads, the tiles to cover as a sub-list of the 128-row table (gn_logits, scan, conv_igemm
// up to 32 classes) and of the head_BM-row table (conv_igemm above), the rows behind the profile FLOPs
struct CondEp {
  const void* wt; const float *bias, *bias_scan; int N;
  const int2 *t32; int n32; const int2* tBM; int nBM;
  double rows;
  float* out = nullptr;  // conv_igemm only: where column 0 of the launch goes (nullptr: Plan::logits; a code set: its first column)
};

// launch e of the head that o describes, to be run by kernel k: episode e of a mixed head over its tile sub-lists, set e of a code-sets
// head into its own columns, or (e = 0) the uniform head; the last two cover the plan's whole tile tables
static CondEp cond_ep(const sylph_ctx* c, const Plan* P, const HeadOut& o, int e, HeadKind k) {
  const bool eps = o.src == HeadOut::episodes, sets = o.src == HeadOut::codesets;
  const PackedCodes& pc = eps ? P->ep.codes : sets ? P->cs.codes : P->codes;
  const size_t r0 = eps ? P->ep.row0[e] : sets ? P->cs.col0[e] : 0;
  const int N = eps ? P->ep.n[e] : sets ? P->cs.n[e] : o.ncls;
  CondEp v = {(const char*)pc.w + r0 * 256 * c->esz(), o.has_bias ? pc.bias + r0 : nullptr, pc.bias + pc.cap + r0, N,
              P->head_tiles32, P->head_mtiles32, P->head_tiles, P->head_mtiles, (double)P->B * P->Ltot, sets ? P->logits + r0 : nullptr};
  if (eps) {
    const int2 a = P->ep.tiles32[e], b = P->ep.tilesBM[e];
    int n_img = 0;
    for (int i : P->ep.image) n_img += i == e;
    const bool fused = k == HeadKind::gn_logits || k == HeadKind::scan;  // (their FLOPs count whole 128-row tiles)
    v.t32 = P->ep.tiles_dev + a.x; v.n32 = a.y; v.tBM = P->ep.tiles_dev + b.x; v.nBM = b.y;
    v.rows = fused ? a.y * 128.0 : (double)n_img * P->Ltot;
  }
  return v;
}

// one launch of kind k into the logits (pitch o.logits_ld) or, scan, into the decode buffers; clear_counts: the first scan of a head
static int launch_cond(sylph_ctx* c, Plan* P, const HeadOut& o, HeadKind k, const CondEp& v, bool clear_counts) {
  const Plan* PP = P;
  const int N = v.N, ld = o.logits_ld;
  const double flops = 2.0 * v.rows * N * 256.0;
  if (k == HeadKind::gn_logits) {
    KCHK(timed_op(c, "gn_logits_kernel", flops, c->stream, [=](hipStream_t st) {
           return launch_gn_logits(PP->src.feat, 256, PP->src.coef, v.wt, v.bias, N, PP->logits, ld, PP->head_segs, v.t32, v.n32, st);
         }), "gn_logits");
    return 0;
  }
  if (k == HeadKind::scan) {
    RET(ensure_decode_slots(c, P, P->dec, P->B, o.ncls));  // (in front of the scan: see there)
    DecodeCfg d = decode_cfg(c, P, P->dec, o, 0);
    d.num_classes = N;
    const int nseg = P->B * c->cfg.nlevels;
    // the counters hold this scan's candidates from here on (set before the launch: a failed one may have counted too): whatever fills
    // the logits next -- a plain head, the pretrained head, an import -- before a decode has run must not have its decode scan append to
    // them (sylph_decode_nms clears a dirty table in front of a plain scan)
    P->cand_dirty = true;
    KCHK(timed_op(c, "logits_scan_kernel", flops, c->stream, [=](hipStream_t st) {
           return launch_logits_scan(PP->src.feat, 256, PP->src.coef, v.wt, PP->code_wf, v.bias_scan, PP->head_segs, v.t32, v.n32, PP->src.pred, 8, d,
                                     PP->dec.buf, nseg, clear_counts, st);
         }), "logits_scan");
    return 0;
  }
  const int bn = cond_pad(N).bn;  // conv_igemm: 128-row tiles up to 32 classes, head_BM-row tiles above
  ConvArgs a;
  memset(&a, 0, sizeof(a));
  a.in = P->cls_feat; a.wt = v.wt; a.out = v.out ? v.out : P->logits;
  a.shift = v.bias;
  a.zeros = c->zeros; a.tap_dy = 1;
  a.segs = P->head_segs;
  int BM = P->head_BM;
  if (bn == 32) { BM = 128; a.tiles = v.t32; a.n_mtiles = v.n32; }
  else { a.tiles = v.tBM; a.n_mtiles = v.nBM; }
  a.n_ntiles = cond_pad(N).Npad / bn;
  a.Cin = 256; a.Cout = N; a.KH = 1; a.KW = 1; a.stride = 1; a.pad = 0;
  a.in_ld = 256; a.out_ld = ld;
  const DType dt = c->dt;
  KCHK(timed_op(c, "conv_igemm_kernel", flops, c->stream, [=](hipStream_t st) { return launch_conv(dt, true, a, BM, bn, st); }), "cond_cls_logits");
  return 0;
}

// The launches of the uniform head (one) or of a mixed head (one per episode that has images), each with the kernel head_kind picks for its
// N.  missing_only: only the episodes whose logits a scan left out, with the unfused kernel (sylph_export_head).
struct CondLaunch { HeadKind k; CondEp v; };
static std::vector<CondLaunch> cond_launches(const sylph_ctx* c, const Plan* P, const HeadOut& o, bool missing_only) {
  std::vector<CondLaunch> list;
  const int E = o.src == HeadOut::episodes ? (int)P->ep.n.size() : 1;
  for (int e = 0; e < E; ++e) {
    const int N = o.src == HeadOut::episodes ? P->ep.n[e] : o.ncls;
    if (missing_only && head_kind(c, P, N) != HeadKind::scan) continue;
    const HeadKind k = head_kind(c, P, N, !missing_only);
    const CondEp v = cond_ep(c, P, o, e, k);
    if (v.n32 != 0) list.push_back({k, v});  // (0: an episode no image uses)
  }
  return list;
}

// does every launch of `list` read the tower output through pointers, un-normalised (run_towers)?
static bool all_streaming(const std::vector<CondLaunch>& list) {
  for (const CondLaunch& l : list)
    if (l.k != HeadKind::gn_logits && l.k != HeadKind::scan) return false;
  return true;
}

// Runs the class-conditional convs `list` of the head that o describes -> *scanned: some launch left candidates instead of logits.  The
// last cls GroupNorm is applied in place, ONCE, and only after every kernel that reads the un-normalised tower output (gn_logits, scan; the
// caller's gn_logits_sets launches) has been launched: the conv_igemm launches that need it come last, in list order.  record_apply: the
// apply gets a profile record of its own (the code-sets head's does).
static int run_cond(sylph_ctx* c, Plan* P, const HeadOut& o, const std::vector<CondLaunch>& list, bool record_apply, bool* scanned) {
  bool applied = false, any_scan = false;
  for (int pass = 0; pass < 2; ++pass)
    for (const CondLaunch& l : list) {
      if ((l.k == HeadKind::igemm_after_apply) != (pass == 1)) continue;
      if (pass == 1 && !applied) {
        if (record_apply) RET(apply_cls_gn(c, P));
        else { P->cls_applied = true; KCHK(P->cls_apply(c->stream), "gn_apply (cls tower, last layer)"); }
        applied = true;
      }
      RET(launch_cond(c, P, o, l.k, l.v, !any_scan));
      any_scan = any_scan || l.k == HeadKind::scan;
    }
  if (scanned) *scanned = any_scan;
  return 0;
}

// ---- several code sets over the same images (sylph_fcos_head_codesets / sylph_decode_nms_codesets) ------------------------------------

// does set size N take the fused GroupNorm + conv kernel (gn_logits_sets_kernel)?  Exactly where sylph_fcos_head writes its logits with
// gn_logits_kernel; every other set runs conv_igemm as there (after the deferred GroupNorm apply where the head ops left it out).  The
// fused conv + score scan is not used per set: its detections equal the logits route's (tests/test_head_sweeps_gpu.py).
static bool set_is_hot(const sylph_ctx* c, const Plan* P, int N) { return head_kind(c, P, N, false) == HeadKind::gn_logits; }

// Host and device tables of a code-sets head: column layout (Plan::cs.col0), packed-row -> source-row table, the decode's segment table
// of G * B slots.  Rebuilt only when n_classes differs from the previous call's on this plan.
static int cs_tables(sylph_ctx* c, Plan* P, int G, const int* n_classes) {
  const int L = c->cfg.nlevels, B = P->B;
  std::vector<int> n(n_classes, n_classes + G);
  Plan::CodeSets& T = P->cs;
  if (T.dsegs && n == T.n) return 0;
  T.n.clear();  // (a failure below leaves no key that would match half-written tables)
  std::vector<int> col0(G, 0), src0(G, 0);
  int col = 0, src = 0;
  for (int g = 0; g < G; ++g) { src0[g] = src; src += n[g]; }
  bool any_cold = false;
  for (int g = 0; g < G; ++g) {
    if (!set_is_hot(c, P, n[g])) { any_cold = true; continue; }
    col0[g] = col;
    col += (n[g] + 3) & ~3;
  }
  const int hot_blocks = (col + 31) / 32, hot_width = col > 0 && col < 8 ? 8 : col;
  int rows = hot_blocks * 32;
  for (int g = 0; g < G; ++g) {
    if (set_is_hot(c, P, n[g])) continue;
    col0[g] = rows;
    rows += cond_pad(n[g]).Npad;
  }
  const int ld = any_cold ? rows : hot_width;
  std::vector<int> src_row((size_t)rows, -1);
  for (int g = 0; g < G; ++g)
    for (int r = 0; r < n[g]; ++r) src_row[(size_t)col0[g] + r] = src0[g] + r;
  const std::vector<DecodeSeg> base = decode_segs(c, P, nullptr);
  std::vector<DecodeSeg> ds;
  ds.reserve((size_t)G * base.size());
  for (int g = 0; g < G; ++g)
    for (DecodeSeg d : base) {
      d.ncls = n[g]; d.cls0 = col0[g]; d.slot = g * B + d.image;
      ds.push_back(d);
    }
  RET(upload_codes(c, T.codes, src_row));
  RET(grow_dev(c, &T.dsegs, &T.dsegs_cap, G * B * L, sizeof(DecodeSeg)));
  HIPCHK(hipMemcpy(T.dsegs, ds.data(), ds.size() * sizeof(DecodeSeg), hipMemcpyHostToDevice));
  T.col0 = col0; T.hot_blocks = hot_blocks; T.hot_width = hot_width; T.ld = ld;
  T.n = n;
  return 0;
}

// postprocess scales of a decode call -> Plan::img_out_dev; the H2D copy is skipped when they equal what the device table already holds
// (every step of a steady query stream).  Otherwise img_out_host is rewritten: wait only for the previous H2D copy of it, not for the stream
static int upload_img_out(sylph_ctx* c, Plan* P, const int* oh, const int* ow) {
  std::vector<ImageOut> io((size_t)P->B);
  for (int b = 0; b < P->B; ++b) {
    const int H = oh ? oh[b] : P->img_h[b], W = ow ? ow[b] : P->img_w[b];
    // detector_postprocess: python-double ratios cast to the fp32 tensor dtype
    io[b].sx = (float)((double)W / (double)P->img_w[b]);
    io[b].sy = (float)((double)H / (double)P->img_h[b]);
    io[b].out_w = (float)W;
    io[b].out_h = (float)H;
  }
  if (!P->img_out_ev || P->img_out_last.size() != io.size() || memcmp(P->img_out_last.data(), io.data(), io.size() * sizeof(ImageOut)) != 0) {
    if (P->img_out_ev) HIPCHK(hipEventSynchronize(P->img_out_ev));
    else HIPCHK(hipEventCreateWithFlags(&P->img_out_ev, hipEventDisableTiming));
    memcpy(P->img_out_host, io.data(), io.size() * sizeof(ImageOut));
    HIPCHK(hipMemcpyAsync(P->img_out_dev, P->img_out_host, sizeof(ImageOut) * P->B, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipEventRecord(P->img_out_ev, c->stream));
    P->img_out_last = io;
  }
  return 0;
}

}  // namespace sylph_host

extern "C" {

// every head entry: Plan::out = HeadOut() first, the work, then ONE assignment of the whole record as its last action (HeadOut)
int sylph_import_head(sylph_ctx* c, int N, int level, const float* logits, const float* reg, const float* ctr, const float* iou) {
  Plan* P = c->cur;
  if (!P) return fail("no current batch");
  if (N <= 0) return fail("class_code is empty");
  if (level < 0 || level >= c->cfg.nlevels) return fail("bad level");
  OwnerScope own(c, P);
  begin_fresh_batch(c, P);  // (pred is the caller's from here on: no longer what the towers left)
  const HeadOut prev = P->out;
  P->out = HeadOut();
  BUILD(build_head(c, P), P);
  P->src.feat = P->cls_feat; P->src.coef = P->cls_coef; P->src.pred = P->pred;
  HeadOut o;
  o.src = HeadOut::imported;
  if (P->logits && N == prev.ncls && prev.src != HeadOut::codesets) { o.ncls = N; o.logits_ld = prev.logits_ld; }  // level by level into the buffer as the last head laid it out
  else RET(ensure_logits(c, P, N, false, &o));
  const int hw = P->hl[level] * P->wl[level];
  for (int b = 0; b < P->B; ++b) {
    const int row0 = b * P->Ltot + P->off[level];
    if (logits) KCHK(launch_import_nchw(DT_F32, logits + (size_t)b * N * hw, P->logits, N, hw, row0, o.logits_ld, c->stream), "import logits");
    if (reg) KCHK(launch_import_nchw(DT_F32, reg + (size_t)b * 4 * hw, P->pred, 4, hw, row0, 8, c->stream), "import reg");
    if (ctr) KCHK(launch_import_nchw(DT_F32, ctr + (size_t)b * hw, P->pred + 4, 1, hw, row0, 8, c->stream), "import ctr");
    if (iou) KCHK(launch_import_nchw(DT_F32, iou + (size_t)b * hw, P->pred + 5, 1, hw, row0, 8, c->stream), "import iou");
  }
  P->out = o;
  return 0;
}

int sylph_fcos_head(sylph_ctx* c, const float* cls_conv, const float* cls_bias, int N) {
  Plan* P = c->cur;
  if (!P) return fail("no current batch");
  if (N <= 0) return fail("class_code is empty");
  if (!cls_conv) return fail("cls_conv is NULL");
  OwnerScope own(c, P);
  P->out = HeadOut();
  BUILD(build_head(c, P), P);
  if (c->cfg.cg_code_ksize == 3) return fcos_head_3x3(c, P, cls_conv, cls_bias, N);
  HeadOut o;
  o.src = HeadOut::cond;
  o.has_bias = c->cfg.cond_use_bias && cls_bias;
  RET(ensure_logits(c, P, N, true, &o));
  PackedCodes& pc = P->codes;
  RET(ensure_codes(c, pc, cond_pad(N).Npad, 256 * c->esz(), false));
  // one launch: packed codes + biases zero-padded to the packed code rows (device copy: the caller's buffer need not outlive this call) +
  // the -inf padded copy the fused scan reads
  // (in FRONT of the towers: it depends on the caller's codes only, and at small batches the main stream waits for the bbox tower on the
  // side stream at the end of the head ops anyway -- behind them it was 5 us of the step's serial tail)
  KCHK(launch_pack_codes(c->dt, cls_conv, N, 256, pc.rows, pc.w, o.has_bias ? cls_bias : nullptr, pc.bias, pc.bias + pc.cap, c->stream), "pack_codes");
  const std::vector<CondLaunch> list = cond_launches(c, P, o, false);
  RET(run_towers(c, P, all_streaming(list)));
  bool scanned = false;
  RET(run_cond(c, P, o, list, false, &scanned));
  o.logits_missing = scanned;
  o.cand = scanned ? HeadOut::cand_all : HeadOut::cand_none;
  P->out = o;
  return 0;
}

int sylph_fcos_head_episodes(sylph_ctx* c, int E, const float* cls_conv, const float* cls_bias, const int* n_classes, const int* image_episode) {
  Plan* P = c->cur;
  if (!P) return fail("no current batch");
  if (c->cfg.cg_code_ksize != 1)
    return fail("sylph_fcos_head_episodes runs 1x1 class codes only (CODE_GENERATOR.CLS_LAYER kernel size " + std::to_string(c->cfg.cg_code_ksize) +
                " is not supported here; use sylph_fcos_head per episode)");
  if (E <= 0) return fail("no episodes (E <= 0)");
  if (!cls_conv) return fail("cls_conv is NULL");
  if (!n_classes || !image_episode) return fail("n_classes / image_episode is NULL");
  int maxN = 0;
  for (int e = 0; e < E; ++e) {
    if (n_classes[e] <= 0) return fail("class_code is empty (episode " + std::to_string(e) + ")");
    if (n_classes[e] > maxN) maxN = n_classes[e];
  }
  for (int b = 0; b < P->B; ++b)
    if (image_episode[b] < 0 || image_episode[b] >= E)
      return fail("image_episode[" + std::to_string(b) + "] = " + std::to_string(image_episode[b]) + " is not in [0, " + std::to_string(E) + ")");
  OwnerScope own(c, P);
  P->out = HeadOut();
  BUILD(build_head(c, P), P);
  HeadOut o;
  o.src = HeadOut::episodes;
  o.has_bias = c->cfg.cond_use_bias && cls_bias;
  RET(ensure_logits(c, P, maxN, true, &o));  // row pitch, candidate capacity and export width: those of the widest episode
  RET(ep_tables(c, P, E, n_classes, image_episode));
  // one launch packs every episode's codes and biases (in front of the towers, as in sylph_fcos_head)
  const PackedCodes& pc = P->ep.codes;
  KCHK(launch_pack_codes_episodes(c->dt, cls_conv, pc.src_row, pc.rows, 256, pc.w, o.has_bias ? cls_bias : nullptr, pc.bias, pc.bias + pc.cap, c->stream),
       "pack_codes_episodes");
  const bool one_launch = head_kind(c, P, maxN) == HeadKind::gn_logits;
  const std::vector<CondLaunch> list = one_launch ? std::vector<CondLaunch>() : cond_launches(c, P, o, false);
  RET(run_towers(c, P, all_streaming(list)));
  bool scanned = false;
  if (one_launch) {
    // every episode takes gn_logits: ONE launch for the whole batch, whatever E is (head_fused.hip)
    const Plan* PP = P;
    const float* bias = o.has_bias ? pc.bias : nullptr;
    const int ld = o.logits_ld;
    KCHK(timed_op(c, "gn_logits_episodes_kernel", 2.0 * (double)P->B * P->Ltot * maxN * 256.0, c->stream, [=](hipStream_t st) {
           return launch_gn_logits_episodes(PP->src.feat, 256, PP->src.coef, PP->ep.codes.w, bias, PP->ep.seg_row0, PP->logits, ld,
                                            PP->head_segs, PP->head_tiles32, PP->head_mtiles32, st);
         }), "gn_logits_episodes");
  } else {
    RET(run_cond(c, P, o, list, false, &scanned));
  }
  o.logits_missing = scanned;
  o.cand = scanned ? HeadOut::cand_scanned : HeadOut::cand_none;
  P->out = o;
  return 0;
}

int sylph_fcos_head_pretrained(sylph_ctx* c, int* num_classes) {
  Plan* P = c->cur;
  if (!P) return fail("no current batch");
  if (!c->has_cls_logits) return fail("the checkpoint has no proposal_generator.fcos_head.cls_logits (1x1 or 3x3, 256 input channels)");
  OwnerScope own(c, P);
  P->out = HeadOut();
  BUILD(build_head(c, P), P);
  const int N = c->cls_logits.Cout;
  HeadOut o;
  o.src = HeadOut::pretrained;
  RET(ensure_logits(c, P, N, false, &o));
  if (c->cls_logits.Cout_pad != o.logits_ld) return fail("internal: cls_logits padding");
  if (P->cls_logits_dst != P->logits) {  // (re)build the conv launch for this plan's buffers
    P->cls_logits_ops.clear();
    ConvOpts op; op.pad = c->cls_logits.KH / 2; op.segs_per_image = c->cfg.nlevels; op.out_f32 = true;
    RET(add_conv(c, P->cls_logits_ops, c->cls_logits, P->cls_feat, 256, P->logits, o.logits_ld, pyramid_segs(c, P), op));
    P->cls_logits_dst = P->logits;
  }
  RET(run_towers(c, P, false));
  if (P->cls_coef) RET(apply_cls_gn(c, P));
  RET(run_ops(c, P->cls_logits_ops, "cls_logits"));
  if (num_classes) *num_classes = N;
  P->out = o;
  return 0;
}

int sylph_export_head(sylph_ctx* c, int level, float* logits, float* reg, float* ctr, float* iou) {
  Plan* P = c->cur;
  if (!P || P->out.src == HeadOut::none) return fail("sylph_fcos_head must be called first");
  if (level < 0 || level >= c->cfg.nlevels) return fail("bad level");
  if (logits && P->out.logits_missing) {  // a fused scan left columns out: the unfused conv writes them now, and the record says so
    OwnerScope own(c, P);
    HeadOut o = P->out;
    P->out = HeadOut();
    if (c->rec) RET(restore_record(c, P));  // (the unfused conv normalises in place: on the plan's copy, never in the record)
    RET(run_cond(c, P, o, cond_launches(c, P, o, true), false, nullptr));
    o.logits_missing = false;
    P->out = o;
  }
  const HeadOut& o = P->out;
  const int hw = P->hl[level] * P->wl[level];
  int sumN = 0;  // code sets: logits (B, sum N_g, h, w), set after set
  if (o.src == HeadOut::codesets)
    for (int n : P->cs.n) sumN += n;
  for (int b = 0; b < P->B; ++b) {
    const int row0 = b * P->Ltot + P->off[level];
    if (logits && o.src == HeadOut::codesets) {
      size_t ch = 0;
      for (size_t g = 0; g < P->cs.n.size(); ++g) {
        KCHK(launch_export_nchw_f32(P->logits, logits + ((size_t)b * sumN + ch) * hw, P->cs.n[g], hw, row0, o.logits_ld, P->cs.col0[g], c->stream),
             "export logits");
        ch += (size_t)P->cs.n[g];
      }
    } else if (logits)
      KCHK(launch_export_nchw_f32(P->logits, logits + (size_t)b * o.ncls * hw, o.ncls, hw, row0, o.logits_ld, 0, c->stream), "export logits");
    if (reg) KCHK(launch_export_nchw_f32(P->src.pred, reg + (size_t)b * 4 * hw, 4, hw, row0, 8, 0, c->stream), "export reg");
    if (ctr) KCHK(launch_export_nchw_f32(P->src.pred, ctr + (size_t)b * hw, 1, hw, row0, 8, 4, c->stream), "export ctr");
    if (iou) KCHK(launch_export_nchw_f32(P->src.pred, iou + (size_t)b * hw, 1, hw, row0, 8, 5, c->stream), "export iou");
  }
  return 0;
}

int sylph_decode_nms(sylph_ctx* c, const int* oh, const int* ow, int max_out, float* boxes, float* scores,
                     int* classes, int* levels, float* locations, int* cand, int* counts, int* status) {
  Plan* P = c->cur;
  if (!P || P->out.src == HeadOut::none) return fail("sylph_fcos_head must be called first");
  if (max_out <= 0) return fail("max_out must be positive");
  if (P->out.src == HeadOut::codesets)  // (its G * B result slots would overrun the caller's B-sized buffers)
    return fail("the last head call was sylph_fcos_head_codesets (" + std::to_string(P->out.nsets) + " code sets): decode it with sylph_decode_nms_codesets");
  const HeadOut o = P->out;
  OwnerScope own(c, P);
  RET(ensure_decode_slots(c, P, P->dec, P->B, o.ncls));
  RET(upload_img_out(c, P, oh, ow));
  const DecodeCfg d = decode_cfg(c, P, P->dec, o, max_out);
  const int L = c->cfg.nlevels;
  // the three states of HeadOut::cand: clear stale counters in front of a scan of every image, or keep the candidates that are there
  if (o.cand == HeadOut::cand_none && P->cand_dirty) HIPCHK(hipMemsetAsync(P->dec.buf.cand_count, 0, (size_t)P->B * L * 4, c->stream));
  P->cand_dirty = o.cand != HeadOut::cand_none;
  int nwb = (L * c->cfg.pre_nms_topk + 63) / 64;
  if (nwb > P->pool_cap / 64) nwb = P->pool_cap / 64;
  KCHK(launch_decode(d, o.src == HeadOut::episodes ? P->ep.dsegs : P->dsegs, P->B * L, P->hl[0] * P->wl[0], P->B, nwb, P->logits, P->src.pred, 8,
                     P->dec.buf, P->img_out_dev, boxes, scores, classes, levels, locations, cand, counts, status, o.cand == HeadOut::cand_all, c->stream),
       "decode_nms");
  return 0;
}

/* see include/sylph_hip.h */
int sylph_fcos_head_codesets(sylph_ctx* c, int G, const float* cls_conv, const float* cls_bias, const int* n_classes) {
  Plan* P = c->cur;
  if (!P) return fail("no current batch");
  if (c->cfg.cg_code_ksize != 1)
    return fail("sylph_fcos_head_codesets runs 1x1 class codes only (CODE_GENERATOR.CLS_LAYER kernel size " + std::to_string(c->cfg.cg_code_ksize) +
                " is not supported here; use sylph_fcos_head per code set)");
  if (G <= 0) return fail("no code sets (G <= 0)");
  if (!cls_conv) return fail("cls_conv is NULL");
  if (!n_classes) return fail("n_classes is NULL");
  int maxN = 0;
  long sumN = 0;
  for (int g = 0; g < G; ++g) {
    if (n_classes[g] <= 0) return fail("class_code is empty (code set " + std::to_string(g) + ")");
    if (n_classes[g] > maxN) maxN = n_classes[g];
    sumN += n_classes[g];
  }
  if (sumN + 128L * G > (1L << 20)) return fail("the code sets hold " + std::to_string(sumN) + " classes: too many for one logits row");
  OwnerScope own(c, P);
  P->out = HeadOut();
  BUILD(build_head(c, P), P);
  HeadOut o;
  o.src = HeadOut::codesets;
  o.has_bias = c->cfg.cond_use_bias && cls_bias;
  o.nsets = G;
  o.ncls = maxN;  // candidate capacity per (slot, level): that of the widest set
  RET(cs_tables(c, P, G, n_classes));
  const Plan::CodeSets& T = P->cs;
  const PackedCodes& pc = T.codes;
  o.logits_ld = T.ld;
  RET(grow_dev(c, &P->logits, &P->logits_cap_ld, T.ld, (size_t)P->B * P->Ltot * sizeof(float)));  // all sets' logits stay resident until the decode
  // one launch packs every set's codes and biases (in front of the towers, as in sylph_fcos_head)
  KCHK(launch_pack_codes_episodes(c->dt, cls_conv, pc.src_row, pc.rows, 256, pc.w, o.has_bias ? cls_bias : nullptr, pc.bias, pc.bias + pc.cap, c->stream),
       "pack_codes (code sets)");
  std::vector<CondLaunch> cold;  // every set that does not take gn_logits_sets_kernel, in order g
  for (int g = 0; g < G; ++g)
    if (!set_is_hot(c, P, n_classes[g])) {
      const HeadKind k = head_kind(c, P, n_classes[g], false);
      cold.push_back({k, cond_ep(c, P, o, g, k)});
    }
  RET(run_towers(c, P, cold.empty()));  // towers, box heads, cls GroupNorm statistics: once, whatever G is
  const Plan* PP = P;
  const int ld = T.ld;
  // the sets of up to 32 classes: GN_SETS_MAX_BLOCKS blocks of 32 packed rows per pass over the un-normalised tower output
  for (int b0 = 0; b0 < T.hot_blocks; b0 += GN_SETS_MAX_BLOCKS) {
    const int nb = T.hot_blocks - b0 < GN_SETS_MAX_BLOCKS ? T.hot_blocks - b0 : GN_SETS_MAX_BLOCKS;
    const int width = T.hot_width - 32 * b0 < 32 * nb ? T.hot_width - 32 * b0 : 32 * nb;
    KCHK(timed_op(c, "gn_logits_sets_kernel", 2.0 * (double)P->head_mtiles32 * 128.0 * width * 256.0, c->stream, [=](hipStream_t st) {
           return launch_gn_logits_sets(PP->src.feat, 256, PP->src.coef, (const char*)pc.w + (size_t)32 * b0 * 256 * 2, pc.bias + 32 * b0, nb,
                                        PP->logits + 32 * b0, ld, width, PP->head_segs, PP->head_tiles32, PP->head_mtiles32, st);
         }), "gn_logits_sets");
  }
  // every other set, in order g: the conv_igemm launch sylph_fcos_head gives its N, on the tower output normalised in place ONCE, after
  // the kernel above has read the un-normalised one (run_cond)
  RET(run_cond(c, P, o, cold, true, nullptr));
  o.cand = HeadOut::cand_none;
  P->out = o;
  return 0;
}

/* see include/sylph_hip.h */
int sylph_decode_nms_codesets(sylph_ctx* c, int G, const int* oh, const int* ow, int max_out, float* boxes, float* scores, int* classes,
                              int* levels, float* locations, int* cand, int* counts, int* status) {
  Plan* P = c->cur;
  if (!P || P->out.src == HeadOut::none) return fail("sylph_fcos_head_codesets must be called first");
  if (P->out.src != HeadOut::codesets)
    return fail("the last head call was not sylph_fcos_head_codesets: decode it with sylph_decode_nms");
  if (max_out <= 0) return fail("max_out must be positive");
  const HeadOut o = P->out;
  if (G != o.nsets)
    return fail("sylph_decode_nms_codesets: G = " + std::to_string(G) + ", but the last sylph_fcos_head_codesets call ran " + std::to_string(o.nsets) +
                " code sets");
  OwnerScope own(c, P);
  const int L = c->cfg.nlevels, slots = G * P->B;
  RET(ensure_decode_slots(c, P, P->dec_cs, slots, o.ncls));
  RET(upload_img_out(c, P, oh, ow));
  const DecodeCfg d = decode_cfg(c, P, P->dec_cs, o, max_out);
  KCHK(launch_decode(d, P->cs.dsegs, slots * L, P->hl[0] * P->wl[0], slots, 0, P->logits, P->src.pred, 8, P->dec_cs.buf, P->img_out_dev, boxes, scores,
                     classes, levels, locations, cand, counts, status, false, c->stream),
       "decode_nms_codesets");
  return 0;
}

/* see include/sylph_hip.h */
int sylph_fcos_towers(sylph_ctx* c) {
  Plan* P = c->cur;
  if (!P) return fail("no current batch");
  RET(refuse_on_record(c, "sylph_fcos_towers"));
  OwnerScope own(c, P);
  P->out = HeadOut();  // no logits: a decode or an export answers "sylph_fcos_head must be called first"
  BUILD(build_head(c, P), P);
  return run_towers(c, P, true);
}

/* see include/sylph_hip.h */
int sylph_record_store(sylph_ctx* c, sylph_record** out) {
  if (!out) return fail("sylph_record_store: out is NULL");
  *out = nullptr;
  Plan* P = c->cur;
  if (!P) return fail("no current batch");
  if (c->rec) return fail("sylph_record_store: the current batch is a query record already");
  if (!P->head_built || !P->towers_fresh)
    return fail("sylph_record_store: the towers have not run on the current batch (call sylph_fcos_towers or a head entry first)");
  if (P->cls_coef && P->cls_applied)
    return fail("sylph_record_store: an earlier head call on this batch applied the cls tower's last GroupNorm in place (igemm_after_apply, the "
                "pretrained head, or a logits export after a fused scan): the tower output is no longer the one the streaming kernels read; "
                "run sylph_fcos_towers again first");
  if (P->cls_coef && (!P->cls_gn.coef || !P->cls_gn.partial)) return fail("internal: deferred cls GroupNorm without its tables");
  HIPCHK(hipSetDevice(c->device));
  std::unique_ptr<sylph_record> R(new sylph_record());
  const size_t rows = (size_t)P->B * P->Ltot;
  auto pad = [](size_t n) { return (n + 255) & ~(size_t)255; };
  R->feat_bytes = rows * 256 * c->esz();
  R->pred_bytes = rows * 8 * sizeof(float);
  R->coef_bytes = P->cls_coef ? P->cls_gn.coef_bytes : 0;
  R->partial_bytes = P->cls_coef ? P->cls_gn.partial_bytes : 0;
  const size_t total = pad(R->feat_bytes) + pad(R->pred_bytes) + pad(R->coef_bytes) + pad(R->partial_bytes);
  if (ctx_alloc(c, &R->base, total) != 0)  // eviction never frees a record
    return fail("sylph_record_store: cannot allocate the record's " + std::to_string(total) + " bytes (" + sylph_last_error() + ")");
  char* p = (char*)R->base;
  R->feat = p; p += pad(R->feat_bytes);
  R->pred = (const float*)p; p += pad(R->pred_bytes);
  if (P->cls_coef) {
    R->coef = (const float2*)p; p += pad(R->coef_bytes);
    R->partial = (const float*)p;
  }
  hipError_t e = hipMemcpyAsync(R->base, P->cls_feat, R->feat_bytes, hipMemcpyDeviceToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync((void*)R->pred, P->pred, R->pred_bytes, hipMemcpyDeviceToDevice, c->stream);
  if (e == hipSuccess && R->coef) e = hipMemcpyAsync((void*)R->coef, P->cls_gn.coef, R->coef_bytes, hipMemcpyDeviceToDevice, c->stream);
  if (e == hipSuccess && R->coef) e = hipMemcpyAsync((void*)R->partial, P->cls_gn.partial, R->partial_bytes, hipMemcpyDeviceToDevice, c->stream);
  if (e != hipSuccess) {
    c->dfree(R->base);
    return fail(std::string("sylph_record_store: copy failed: ") + hipGetErrorString(e));
  }
  R->owner = c; R->device = c->device; R->dt = c->dt;
  R->tower_norm = c->cfg.tower_norm; R->nlevels = c->cfg.nlevels; R->code_ksize = c->cfg.cg_code_ksize;
  for (int l = 0; l < 8; ++l) R->strides[l] = c->cfg.strides[l];
  R->B = P->B; R->H = P->H; R->W = P->W;
  R->box_stamp = c->box_stamp;
  R->img_h = P->img_h; R->img_w = P->img_w;
  R->bytes = (int64_t)total;
  c->records.push_back(R.get());
  *out = R.release();
  return 0;
}

/* see include/sylph_hip.h */
int sylph_record_load(sylph_ctx* c, const sylph_record* R) {
  if (!R) return fail("sylph_record_load: the record is NULL");
  if (!c->finalized) return fail("weights not finalized");
  static const char* const dt_name[] = {"f32", "bf16", "f32s"};
  auto dtn = [&](DType d) { return d == DT_BF16 ? dt_name[1] : (d == DT_F32S ? dt_name[2] : dt_name[0]); };
  if (R->device != c->device) return fail("sylph_record_load: the record lives on device " + std::to_string(R->device) + ", the context on " + std::to_string(c->device));
  if (R->dt != c->dt)
    return fail(std::string("sylph_record_load: the record was made under dtype ") + dtn(R->dt) + ", the context runs " + dtn(c->dt));
  bool same = R->tower_norm == c->cfg.tower_norm && R->nlevels == c->cfg.nlevels && R->code_ksize == c->cfg.cg_code_ksize;
  for (int l = 0; l < 8 && same; ++l) same = R->strides[l] == c->cfg.strides[l];
  if (!same)
    return fail("sylph_record_load: the record was made under another sylph_config (tower norm " + std::to_string(R->tower_norm) + ", " +
                std::to_string(R->nlevels) + " levels, first stride " + std::to_string(R->strides[0]) + ", code kernel size " + std::to_string(R->code_ksize) +
                "; the context: " + std::to_string(c->cfg.tower_norm) + ", " + std::to_string(c->cfg.nlevels) + ", " + std::to_string(c->cfg.strides[0]) + ", " +
                std::to_string(c->cfg.cg_code_ksize) + ")");
  if (R->box_stamp != c->box_stamp)
    return fail("sylph_record_load: the record's box / centerness / IoU predictions come from another box branch (stored under branch stamp " +
                std::to_string(R->box_stamp) + ", the context now runs " + std::to_string(c->box_stamp) +
                "; 0 = the finalized tensors): restore that branch (sylph_set_box_branch; three NULLs for the finalized one) or store the record again");
  HIPCHK(hipSetDevice(c->device));
  Plan* P = get_plan(c, R->B, R->H, R->W);
  OwnerScope own(c, P);
  BUILD(build_head(c, P), P);
  if ((size_t)P->B * P->Ltot * 256 * c->esz() != R->feat_bytes || (R->coef != nullptr) != (P->cls_coef != nullptr) ||
      (R->coef && (R->coef_bytes != P->cls_gn.coef_bytes || R->partial_bytes != P->cls_gn.partial_bytes)))
    return fail("sylph_record_load: the record's tower layout is not this context's (the deferred cls GroupNorm or the tile geometry differ)");
  begin_fresh_batch(c, P);  // (leaves an earlier record; P's own towers' outputs may be overwritten by a restore from here on)
  P->out = HeadOut();
  P->img_h = R->img_h; P->img_w = R->img_w;
  c->cur = P;
  c->rec = R;
  return 0;
}

/* see include/sylph_hip.h */
int sylph_record_info(const sylph_record* R, int* B, int* H, int* W, int64_t* bytes) {
  if (!R) return fail("sylph_record_info: the record is NULL");
  if (B) *B = R->B;
  if (H) *H = R->H;
  if (W) *W = R->W;
  if (bytes) *bytes = R->bytes;
  return 0;
}

/* see include/sylph_hip.h */
void sylph_record_destroy(sylph_ctx* c, sylph_record* R) {
  if (!c || !R) return;
  if (c->rec == R) {  // the plan that was scoring it keeps nothing that points into it
    if (c->cur) c->cur->out = HeadOut();
    c->rec = nullptr;
    c->cur = nullptr;
  }
  for (size_t i = 0; i < c->records.size(); ++i)
    if (c->records[i] == R) { c->records[i] = c->records.back(); c->records.pop_back(); break; }
  (void)hipSetDevice(c->device);
  c->dfree(R->base);  // drains the stream first
  delete R;
}

}  // extern "C"
