// Host side of libsylph_hip.so, unit "codegen": support path: ROIAlign, code generators, code normalisation / reduction (sylph_codegen*, sylph_normalize_codes, sylph_reduce_codes).
// No torch types, no CPU compute fallback: every stage is a HIP kernel from this directory.
#include "api_internal.h"

namespace sylph_host {

// Parity taps of the support path (sylph_export_support).  A stage that no later op overwrites is recorded where it is; with debug taps
// on, the others are copied aside by a device-to-device copy right after the op that writes them: the kernels and their launches are
// the same with and without taps.  n = images (npos = 49: [n * 49][ld] maps) or rows (npos = 1); n = 0: the classes of the last call.
static void tap_at(SupportPass* Q, int stage, int index, const void* p, bool f32, int n, int npos, int C = 256, int ld = 256) {
  SupportPass::SupTap t;
  t.p = p; t.f32 = f32; t.n = n; t.npos = npos; t.C = C; t.ld = ld;
  Q->taps[{stage, index}] = t;
}

static int tap_copy(sylph_ctx* c, SupportPass* Q, std::vector<OpFn>& ops, int stage, int index, const void* src, bool f32, int n, int npos) {
  if (!c->debug_taps) return 0;
  const size_t bytes = (size_t)n * npos * 256 * (f32 ? 4 : c->esz());
  void* dst = nullptr;
  RET(c->dalloc(&dst, bytes));
  ops.push_back([=](hipStream_t s) { return (int)hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s); });
  tap_at(Q, stage, index, dst, f32, n, npos);
  return 0;
}

static std::vector<LevelDesc> level_table(sylph_ctx* c, Plan* P) {
  std::vector<LevelDesc> lv;
  for (int b = 0; b < P->B; ++b)
    for (int l = 0; l < c->cfg.nlevels; ++l)
      lv.push_back(LevelDesc{b * P->Ltot + P->off[l], P->hl[l], P->wl[l], 1.0f / (float)c->cfg.strides[l]});
  return lv;
}

// the first op of a support pass: ROIAlign of the call's boxes into Q->roi
static void add_roi_align(Plan* P, SupportPass* Q, DType dt, int L) {
  const void* F = P->F;
  const LevelDesc* lvd = P->lv_dev;
  void* roi = Q->roi;
  const int S = Q->S;
  Q->ops.push_back([=](hipStream_t s) { return launch_roi_align(dt, F, 256, lvd, L, Q->cur_boxes, Q->roi_image_dev, S, 7, roi, s); });
}

// add_conv_gn of a support layer (7x7 maps, applied in place) with its taps: the stored pre-GroupNorm output, the statistics of the
// apply, the applied output
static int support_conv_gn(sylph_ctx* c, SupportPass* Q, std::vector<OpFn>& ops, const ConvLayer& L, const void* in, void* out,
                           const std::vector<SegDesc>& segs, ConvOpts o, const GNLayer& G, int relu, int layer) {
  const int S = Q->S;
  o.want_gn = 1;
  Geom g;
  RET(add_conv(c, ops, L, in, 256, out, L.Cout, segs, o, &g));
  RET(tap_copy(c, Q, ops, SYLPH_SUP_GN_Y, layer, out, false, S, 49));
  const float2* stats = nullptr;
  RET(add_gn_from_partials(c, ops, out, L.Cout, segs, g, G, relu, nullptr, nullptr, &stats));
  SupportPass::SupTap t;
  t.n = S; t.npos = 1; t.stats = stats; t.gamma = G.gamma; t.beta = G.beta;
  Q->taps[{SYLPH_SUP_GN_COEF, layer}] = t;
  return tap_copy(c, Q, ops, SYLPH_SUP_LAYER_OUT, layer, out, false, S, 49);
}

// the pyramid's (image, level) table: one per plan, whichever support pass comes first
static int ensure_level_table(sylph_ctx* c, Plan* P) {
  if (P->lv_dev) return 0;
  std::vector<LevelDesc> lv = level_table(c, P);
  return upload(c, (void**)&P->lv_dev, lv.data(), lv.size() * sizeof(LevelDesc));
}

// Q: the pass to build, for S = R rows (row r = ROI r of the call's list).  ROIAlign reads the call's image table (which image a row
// samples), the tail its segment table (which consecutive rows make a code); the convolutions between them run on
// image_segs(S, 7, 7, 7, 7), so their routes follow the row count.
int build_support(sylph_ctx* c, Plan* P, SupportPass* Q) {
  if (Q->built) return 0;
  if (!c->has_codegen) return fail("code generator weights were not loaded");
  RET(ensure_pyramid(c, P));
  const size_t e = c->esz();
  const int S = Q->S, L = c->cfg.nlevels, npos = 49;
  RET(ensure_level_table(c, P));
  RET(c->dalloc(&Q->roi, (size_t)S * npos * 256 * e));
  RET(c->dalloc(&Q->cgA, (size_t)S * npos * 256 * e));
  RET(c->dalloc(&Q->cgB, (size_t)S * npos * 256 * e));
  RET(c->dalloc((void**)&Q->cg_conv_out, (size_t)S * npos * 256 * 4));
  RET(c->dalloc((void**)&Q->cg_bias_out, (size_t)S * npos * 4 * (c->cg_naux > 0 ? c->cg_naux : 1)));
  RET(c->dalloc((void**)&Q->cg_wnorm, (size_t)S * 4));
  const std::vector<SegDesc> segs = image_segs(S, 7, 7, 7, 7);
  auto& ops = Q->ops;
  const DType dt = c->dt;
  SupportPass* QQ = Q;
  add_roi_align(P, Q, dt, L);
  tap_at(Q, SYLPH_SUP_ROI, 0, Q->roi, false, S, npos);
  const void* in = Q->roi;
  void* out = Q->cgA;
  for (size_t i = 0; i < c->cg_tower.size(); ++i) {
    // CODE_GENERATOR.TOWER_LAYERS[i] = [norm, activation] (code_generator.py:648-688): conv3x3 + bias, GroupNorm(32) if "GN", ReLU if "ReLU"
    const bool gn = (c->cfg.cg_tower_gn_mask >> i) & 1, relu = (c->cfg.cg_tower_relu_mask >> i) & 1;
    ConvOpts o; o.pad = 1;
    if (gn) {
      RET(support_conv_gn(c, Q, ops, c->cg_tower[i], in, out, segs, o, c->cg_gn[i], relu ? 1 : 0, (int)i));
    } else {
      if (relu) o.relu_nch = 1 << 30;
      RET(add_conv(c, ops, c->cg_tower[i], in, 256, out, 256, segs, o));
      RET(tap_copy(c, Q, ops, SYLPH_SUP_LAYER_OUT, (int)i, out, false, S, npos));
    }
    in = out;
    out = (out == Q->cgA) ? Q->cgB : Q->cgA;
  }
  ConvOpts oc; oc.pad = 1; oc.out_f32 = true;
  RET(add_conv(c, ops, c->cg_cls, in, 256, Q->cg_conv_out, 256, segs, oc));
  const int naux = c->cg_naux;
  if (naux > 0) RET(add_conv(c, ops, c->cg_bias, in, 256, Q->cg_bias_out, naux, segs, oc));
  tap_at(Q, SYLPH_SUP_CONV_OUT, 0, Q->cg_conv_out, true, S, npos);
  if (naux > 0) tap_at(Q, SYLPH_SUP_CONV_OUT, 1, Q->cg_bias_out, true, S, npos, naux, naux);
  Q->n_shot_ops = ops.size();  // what follows looks at segments
  {
    const float *co = Q->cg_conv_out, *bo = Q->cg_bias_out;
    const int l2 = c->cfg.cg_bias_l2_norm, ib = c->cg_ib, iw = c->cg_iw, is = c->cg_is, ks = c->cfg.cg_code_ksize;
    float* wn = Q->cg_wnorm;
    ops.push_back([=](hipStream_t s) {
      return launch_codegen_tail(co, 256, bo, naux > 0 ? naux : 1, ib, iw, is, QQ->seg_dev, QQ->n_seg, QQ->max_len, npos, 256, ks, l2,
                                 QQ->cur_code_out, wn, s);
    });
  }
  Q->built = true;
  return 0;
}

// The ROIEncoder's two head FC stacks on n class tokens cls[n][256] -> codes_out (n, 257): class k -> row k, the weight head at
// column 0, the bias head (+ prior) at column 256.  h: [2][h_rows][hdim] hidden activations, n <= h_rows.  Shared by the support
// pass and sylph_shot_combine.
static int launch_roienc_heads(const sylph_ctx* c, const float* cls, int n, float* h, int h_rows, int hdim, float* codes_out, hipStream_t s) {
  const float prior = -logf((1.f - 0.01f) / 0.01f);  // ROIEncoder hard-codes prior_prob = 0.01 (roi_encoder.py:139-140), whatever MODEL.FCOS.PRIOR_PROB says
  for (int head = 0; head < 2; ++head) {
    const std::vector<sylph_ctx::Lin>& fcs = head == 0 ? c->re.wh : c->re.bh;
    const float* in = cls;
    float* h0 = h + (size_t)head * h_rows * hdim;
    for (size_t k = 0; k < fcs.size(); ++k) {
      const sylph_ctx::Lin& f = fcs[k];
      const bool last = k + 1 == fcs.size();
      int r;
      if (last) {
        r = launch_linear(0, in, f.K, n, f.W, f.b, f.K, f.O, codes_out + (head == 0 ? 0 : 256), 257, 0, head == 1 ? prior : 0.f, s);
      } else {
        r = launch_linear(0, in, f.K, n, f.W, f.b, f.K, f.O, h0, f.O, 1, 0.f, s);
        in = h0;
      }
      if (r != 0) return r;
    }
  }
  return 0;
}

int build_support_roienc(sylph_ctx* c, Plan* P, SupportPass* Q) {
  if (Q->built) return 0;
  if (!c->has_roienc) return fail("ROIEncoder weights were not loaded");
  RET(ensure_pyramid(c, P));
  const size_t e = c->esz();
  // S ROIs = the shots of one or several classes (the segments of the list).  Everything up to the encoder is per shot; the
  // reference's encoder attends over the CLASS axis of a (classes, shots, C) tensor (roi_encoder.py:184-186) and always sees one
  // class per call at inference, i.e. a length-1 sequence: here too a class never sees another one.
  // The pass has two row counts: S = R ROIs for everything per shot, B images for the context, which is a function of the
  // image alone (utils.py:143-165) and is computed once per image; the MS-CAM gate of ROI r reads the context of image roi_image[r].
  const int S = Q->S, B = P->B, L = c->cfg.nlevels, npos = 49;
  RET(ensure_level_table(c, P));
  RET(c->dalloc(&Q->roi, (size_t)S * npos * 256 * e));
  RET(c->dalloc(&Q->cgA, (size_t)S * npos * 256 * e));
  RET(c->dalloc(&Q->cgB, (size_t)S * npos * 256 * e));
  RET(c->dalloc((void**)&Q->re_ctx, (size_t)B * npos * 256 * 4));
  RET(c->dalloc((void**)&Q->re_tok, (size_t)S * 256 * 4));
  RET(c->dalloc((void**)&Q->re_tmp, (size_t)S * 256 * 4));
  int maxhid = 1024;
  for (auto& l : c->re.layers) maxhid = l.l1.O > maxhid ? l.l1.O : maxhid;
  RET(c->dalloc((void**)&Q->re_hid, (size_t)S * maxhid * 4));
  const int hdim = c->cfg.head_fc_dim > 256 ? c->cfg.head_fc_dim : 256;
  RET(c->dalloc((void**)&Q->re_cls, (size_t)S * 256 * 4));
  RET(c->dalloc((void**)&Q->re_h, (size_t)2 * S * hdim * 4));
  const std::vector<SegDesc> segs = image_segs(S, 7, 7, 7, 7);
  auto& ops = Q->ops;
  const DType dt = c->dt;
  const int xbf = dt == DT_BF16 ? 1 : 0;
  SupportPass* QQ = Q;
  auto& R = c->re;
  add_roi_align(P, Q, dt, L);
  {
    const void* F = P->F;
    const LevelDesc* lvd = P->lv_dev;
    float* ctx = Q->re_ctx;
    ops.push_back([=](hipStream_t s) { return launch_adaptive_context(dt, F, 256, lvd, L, B, 7, ctx, s); });
  }
  tap_at(Q, SYLPH_SUP_ROI, 0, Q->roi, false, S, npos);
  tap_at(Q, SYLPH_SUP_CONTEXT, 0, Q->re_ctx, true, B, npos);
  // GroupNorm layers: 0 = box_pooler, 1 + k = tokenizer conv k
  ConvOpts o; o.pad = 1;
  RET(support_conv_gn(c, Q, ops, R.pool_conv, Q->roi, Q->cgA, segs, o, R.pool_gn, 1, 0));
  {
    const float* ctx = Q->re_ctx;
    void* x = Q->cgA;
    const MsCamWeights w = R.cam;
    ops.push_back([=](hipStream_t s) { return launch_mscam(dt, ctx, QQ->roi_image_dev, x, S, w, s); });
  }
  RET(tap_copy(c, Q, ops, SYLPH_SUP_MSCAM, 0, Q->cgA, false, S, npos));
  void* cur = Q->cgA;
  void* nxt = Q->cgB;
  for (size_t k = 0; k < R.tok_conv.size(); ++k) {
    RET(support_conv_gn(c, Q, ops, R.tok_conv[k], cur, nxt, segs, o, R.tok_gn[k], 1, 1 + (int)k));
    std::swap(cur, nxt);
  }
  // tokenizer FC stack: first FC reads the (position-major) activations directly
  float* tok = Q->re_tok;
  float* tmp = Q->re_tmp;
  float* hid = Q->re_hid;
  {
    const sylph_ctx::Lin f0 = R.tok_fc[0];
    const void* x = cur;
    ops.push_back([=](hipStream_t s) { return launch_linear(xbf, x, npos * 256, S, f0.W, f0.b, f0.K, f0.O, tok, 256, 1, 0.f, s); });
    float* a = tok;
    float* b = tmp;
    for (size_t k = 1; k < R.tok_fc.size(); ++k) {
      const sylph_ctx::Lin f = R.tok_fc[k];
      ops.push_back([=](hipStream_t s) { return launch_linear(0, a, 256, S, f.W, f.b, f.K, f.O, b, 256, 1, 0.f, s); });
      std::swap(a, b);
    }
    tok = a;
    tmp = b;
  }
  RET(tap_copy(c, Q, ops, SYLPH_SUP_TOKENS, 0, tok, true, S, 1));
  int layer = 0;
  for (auto& l : R.layers) {
    const sylph_ctx::Lin at = l.attn, l1 = l.l1, l2 = l.l2;
    const GNLayer n1 = l.n1, n2 = l.n2;
    float *x = tok, *t = tmp;
    ops.push_back([=](hipStream_t s) { return launch_linear(0, x, 256, S, at.W, at.b, 256, 256, t, 256, 0, 0.f, s); });
    ops.push_back([=](hipStream_t s) { return launch_add_layernorm(x, t, S, n1.gamma, n1.beta, s); });
    ops.push_back([=](hipStream_t s) { return launch_linear(0, x, 256, S, l1.W, l1.b, l1.K, l1.O, hid, l1.O, 1, 0.f, s); });
    ops.push_back([=](hipStream_t s) { return launch_linear(0, hid, l1.O, S, l2.W, l2.b, l2.K, l2.O, t, 256, 0, 0.f, s); });
    ops.push_back([=](hipStream_t s) { return launch_add_layernorm(x, t, S, n2.gamma, n2.beta, s); });
    RET(tap_copy(c, Q, ops, SYLPH_SUP_TOKENS, ++layer, tok, true, S, 1));
  }
  tap_at(Q, SYLPH_SUP_CLS_TOKENS, 0, Q->re_cls, true, 0, 1);
  Q->n_shot_ops = ops.size();  // what follows looks at segments
  Q->shot_tok = tok;
  {
    float* cls = Q->re_cls;
    float* x = tok;
    ops.push_back([=](hipStream_t s) { return launch_mean_tokens(x, QQ->seg_dev, QQ->n_seg, cls, s); });
    float* h = Q->re_h;
    ops.push_back([=](hipStream_t s) { return launch_roienc_heads(c, cls, QQ->n_seg, h, S, hdim, QQ->cur_code_out, s); });
  }
  Q->built = true;
  return 0;
}

// the ROI list of a call against the batch: every failure names the offending index
static int check_rois(const Plan* P, int R, const float* boxes, const int* roi_image) {
  if (!P || !P->F) return fail("no current batch");
  if (R < 1) return fail("ROI list: R = " + std::to_string(R) + " (at least one ROI is needed)");
  if (!boxes || !roi_image) return fail("NULL argument");
  for (int r = 0; r < R; ++r)
    if (roi_image[r] < 0 || roi_image[r] >= P->B)
      return fail("ROI list: roi_image[" + std::to_string(r) + "] = " + std::to_string(roi_image[r]) + " is outside the batch of " + std::to_string(P->B) + " images");
  return 0;
}

// Host tables of a support call -> device, like the mixed-episode head's tables (api_head.hip ep_tables): uploaded when they differ
// from what the pass holds, so a loop that repeats its list (or its shots on its batch shape) neither uploads nor synchronises.
// seg_len == nullptr (sylph_codegen_shots, which stops in front of the segments): the image table alone; the segment table of the pass
// stays what it is, so a sylph_codegen_rois call that follows with the same list and the segments of the call before uploads nothing.
static int roi_tables(sylph_ctx* c, SupportPass* Q, const int* roi_image, int n_seg, const int* seg_len) {
  const bool same_images = Q->roi_image_dev && (int)Q->roi_image.size() == Q->S && std::equal(Q->roi_image.begin(), Q->roi_image.end(), roi_image);
  if (!seg_len) {
    if (same_images) return 0;
    Q->roi_image.clear();  // (a failure below leaves no key that would match a half-written table)
    HIPCHK(hipStreamSynchronize(c->stream));  // the previous call may still be reading the table
    if (!Q->roi_image_dev) RET(c->dalloc((void**)&Q->roi_image_dev, (size_t)Q->S * sizeof(int)));
    HIPCHK(hipMemcpy(Q->roi_image_dev, roi_image, (size_t)Q->S * sizeof(int), hipMemcpyHostToDevice));
    Q->roi_image.assign(roi_image, roi_image + Q->S);
    ++c->roi_table_uploads;
    return 0;
  }
  if (same_images && Q->seg_dev && (int)Q->seg_len.size() == n_seg && std::equal(Q->seg_len.begin(), Q->seg_len.end(), seg_len))
    return 0;
  Q->roi_image.clear(); Q->seg_len.clear();  // (a failure below leaves no key that would match half-written tables)
  std::vector<int> ri(roi_image, roi_image + Q->S), sl(seg_len, seg_len + n_seg);
  std::vector<int2> sg;
  int r0 = 0, mx = 0;
  for (int j = 0; j < n_seg; ++j) {
    sg.push_back(make_int2(r0, sl[j]));
    r0 += sl[j];
    mx = sl[j] > mx ? sl[j] : mx;
  }
  HIPCHK(hipStreamSynchronize(c->stream));  // the previous call may still be reading the tables
  if (!Q->roi_image_dev) RET(c->dalloc((void**)&Q->roi_image_dev, (size_t)Q->S * sizeof(int)));
  if (!Q->seg_dev) RET(c->dalloc((void**)&Q->seg_dev, (size_t)Q->S * sizeof(int2)));
  HIPCHK(hipMemcpy(Q->roi_image_dev, ri.data(), ri.size() * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(Q->seg_dev, sg.data(), sg.size() * sizeof(int2), hipMemcpyHostToDevice));
  Q->roi_image = ri; Q->seg_len = sl; Q->max_len = mx;
  ++c->roi_table_uploads;
  return 0;
}

// One support call, its arguments checked: the plan's pass for R rows (built on first use), the call's tables, the launches.
static int run_support(sylph_ctx* c, Plan* P, int R, const float* boxes, const int* roi_image, int n_seg, const int* seg_len, float* codes_out,
                       const char* what) {
  HIPCHK(hipSetDevice(c->device));
  OwnerScope own(c, P);
  auto& slot = P->sup[R];
  if (!slot) { slot.reset(new SupportPass()); slot->S = R; }
  SupportPass* Q = slot.get();
  if (c->cfg.cg_type == 1) BUILD(build_support_roienc(c, P, Q), P);
  else BUILD(build_support(c, P, Q), P);
  RET(roi_tables(c, Q, roi_image, n_seg, seg_len));
  Q->cur_boxes = boxes;
  Q->cur_code_out = codes_out;
  Q->n_seg = n_seg;
  P->sup_last = Q;
  return run_ops(c, Q->ops, what);
}

// floats of one shot-bank row under the context's config: the code values of one shot, then bias term | logit | scale term | pad
// (CodeGenerator), or the shot's token and four pad floats (ROIEncoder)
static int shot_row_floats(const sylph_ctx* c) {
  const int k = c->cfg.cg_type == 1 ? 1 : c->cfg.cg_code_ksize;
  return 256 * k * k + 4;
}

// The per-shot part of one support call, its arguments checked: the ops of the plan's pass for R rows in front of its first
// segment-wise op, then the rows.
static int run_shots(sylph_ctx* c, Plan* P, int R, const float* boxes, const int* roi_image, float* rows_out) {
  HIPCHK(hipSetDevice(c->device));
  OwnerScope own(c, P);
  auto& slot = P->sup[R];
  if (!slot) { slot.reset(new SupportPass()); slot->S = R; }
  SupportPass* Q = slot.get();
  if (c->cfg.cg_type == 1) BUILD(build_support_roienc(c, P, Q), P);
  else BUILD(build_support(c, P, Q), P);
  RET(roi_tables(c, Q, roi_image, 0, nullptr));
  Q->cur_boxes = boxes;
  P->sup_last = Q;
  std::vector<OpFn> ops(Q->ops.begin(), Q->ops.begin() + Q->n_shot_ops);
  const int row = shot_row_floats(c);
  if (c->cfg.cg_type == 1) {
    const float* tok = Q->shot_tok;
    ops.push_back([=](hipStream_t s) { return launch_shot_token_rows(tok, R, rows_out, row, s); });
  } else {
    const float *co = Q->cg_conv_out, *bo = Q->cg_bias_out;
    const int naux = c->cg_naux, l2 = c->cfg.cg_bias_l2_norm, ib = c->cg_ib, iw = c->cg_iw, is = c->cg_is, ks = c->cfg.cg_code_ksize;
    ops.push_back([=](hipStream_t s) {
      return launch_shot_pool(co, 256, bo, naux > 0 ? naux : 1, ib, iw, is, R, 49, 256, ks, l2, rows_out, row, s);
    });
  }
  return run_ops(c, ops, "codegen_shots");
}

// the stand-alone ROIAlign entries: R checked rows on a scratch context whose allocations are freed on return
static int roi_align_alone(sylph_ctx* c, Plan* P, int R, const float* boxes, const int* roi_image, float* out, const char* what) {
  struct Scratch {
    sylph_ctx tmp;
    hipStream_t s;
    explicit Scratch(sylph_ctx* c) : s(c->stream) { tmp.device = c->device; tmp.dt = c->dt; tmp.stream = c->stream; tmp.zeros = c->zeros; }
    ~Scratch() { (void)hipStreamSynchronize(s); for (void* p : tmp.allocs) (void)hipFree(p); }
  };
  HIPCHK(hipSetDevice(c->device));
  const std::vector<LevelDesc> lv = level_table(c, P);
  Scratch sc(c);
  LevelDesc* lvd = nullptr;
  int* rid = nullptr;
  void* roi = nullptr;
  RET(upload(&sc.tmp, (void**)&lvd, lv.data(), lv.size() * sizeof(LevelDesc)));
  RET(upload(&sc.tmp, (void**)&rid, roi_image, (size_t)R * sizeof(int)));
  RET(sc.tmp.dalloc(&roi, (size_t)R * 49 * 256 * c->esz()));
  KCHK(launch_roi_align(c->dt, P->F, 256, lvd, c->cfg.nlevels, boxes, rid, R, 7, roi, c->stream), what);
  for (int r = 0; r < R; ++r)
    KCHK(launch_export_nchw(c->dt, roi, out + (size_t)r * 256 * 49, 256, 49, r * 49, 256, c->stream), "export roi");
  return 0;
}

// roi_image of the one-box-per-image form: row r is image r
static std::vector<int> identity_images(int B) {
  std::vector<int> v(B);
  for (int b = 0; b < B; ++b) v[b] = b;
  return v;
}

}  // namespace sylph_host

extern "C" {

int sylph_roi_align(sylph_ctx* c, const float* boxes, float* out) {
  RET(refuse_on_record(c, "sylph_roi_align"));
  Plan* P = c->cur;
  if (!P || !P->F) return fail("no current batch");
  if (!boxes || !out) return fail("NULL argument");
  return roi_align_alone(c, P, P->B, boxes, identity_images(P->B).data(), out, "roi_align");
}

int sylph_roi_align_rois(sylph_ctx* c, int R, const float* boxes, const int* roi_image, float* out) {
  RET(refuse_on_record(c, "sylph_roi_align_rois"));
  Plan* P = c->cur;
  RET(check_rois(P, R, boxes, roi_image));
  if (!out) return fail("NULL argument");
  return roi_align_alone(c, P, R, boxes, roi_image, out, "roi_align_rois");
}

/* see include/sylph_hip.h */
int sylph_roi_rows(sylph_ctx* c, int R, const float* boxes_dev, const int* roi_image, void* rows_out_dev) {
  RET(refuse_on_record(c, "sylph_roi_rows"));
  if (c->dt != DT_BF16)
    return fail(std::string("sylph_roi_rows: the ROI bank is bf16 (this context: ") + (c->dt == DT_F32S ? "f32s" : "fp32") + " storage)");
  Plan* P = c->cur;
  RET(check_rois(P, R, boxes_dev, roi_image));
  if (!rows_out_dev) return fail("NULL argument");
  if (R > 65535) return fail("ROI list: R = " + std::to_string(R) + " ROIs in one call; at most 65535");
  HIPCHK(hipSetDevice(c->device));
  {
    OwnerScope own(c, P);
    RET(ensure_level_table(c, P));
  }
  if ((size_t)R > c->roi_rows_cap) {  // the call's image table: the context's, grown on demand
    OwnerScope ctx_owned(c, nullptr);
    if (c->roi_rows_img) c->dfree(c->roi_rows_img);
    c->roi_rows_img = nullptr; c->roi_rows_cap = 0;
    RET(c->dalloc((void**)&c->roi_rows_img, (size_t)R * 2 * sizeof(int)));
    c->roi_rows_cap = (size_t)R * 2;
  }
  HIPCHK(hipStreamSynchronize(c->stream));  // the previous call may still be reading the table
  HIPCHK(hipMemcpy(c->roi_rows_img, roi_image, (size_t)R * sizeof(int), hipMemcpyHostToDevice));
  KCHK(launch_roi_align(c->dt, P->F, 256, P->lv_dev, c->cfg.nlevels, boxes_dev, c->roi_rows_img, R, 7, rows_out_dev, c->stream), "roi_rows");
  return 0;
}

static int support_tap(sylph_ctx* c, int stage, int index, const SupportPass::SupTap** t, int* n) {
  Plan* P = c->cur;
  const SupportPass* Q = P ? P->sup_last : nullptr;
  if (!Q || !Q->built) return fail("no code-generator pass on the current batch");
  auto it = Q->taps.find({stage, index});
  if (it == Q->taps.end())
    return fail("support tap (" + std::to_string(stage) + ", " + std::to_string(index) + ") does not exist in this configuration" +
                (c->debug_taps ? "" : " (intermediate stages need sylph_set_debug_taps(1) before the first code-generator call of a batch shape)"));
  *t = &it->second;
  *n = it->second.n > 0 ? it->second.n : Q->n_seg;
  return 0;
}

int sylph_support_tap_numel(sylph_ctx* c, int stage, int index, int64_t* numel) {
  const SupportPass::SupTap* t;
  int n;
  RET(support_tap(c, stage, index, &t, &n));
  *numel = t->stats ? (int64_t)n * 512 : (int64_t)n * t->C * t->npos;
  return 0;
}

int sylph_export_support(sylph_ctx* c, int stage, int index, float* out) {
  const SupportPass::SupTap* t;
  int n;
  RET(support_tap(c, stage, index, &t, &n));
  if (!out) return fail("NULL argument");
  HIPCHK(hipSetDevice(c->device));
  if (t->stats) {  // (a, b) = (rstd * gamma, fma(-mean, a, beta)) per (image, channel), as gn_apply_partials_kernel forms them (contracted)
    std::vector<float2> st((size_t)n * 32);
    std::vector<float> ga(256), be(256), ab((size_t)n * 512);
    HIPCHK(hipMemcpyAsync(st.data(), t->stats, st.size() * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(ga.data(), t->gamma, 256 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(be.data(), t->beta, 256 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int s = 0; s < n; ++s)
      for (int ch = 0; ch < 256; ++ch) {
        const float2 v = st[(size_t)s * 32 + ch / 8];
        const float a = v.y * ga[ch];
        ab[((size_t)s * 256 + ch) * 2] = a;
        ab[((size_t)s * 256 + ch) * 2 + 1] = fmaf(-v.x, a, be[ch]);
      }
    HIPCHK(hipMemcpyAsync(out, ab.data(), ab.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
  }
  if (t->npos == 1) {  // fp32 rows
    HIPCHK(hipMemcpy2DAsync(out, (size_t)t->C * 4, t->p, (size_t)t->ld * 4, (size_t)t->C * 4, n, hipMemcpyDeviceToDevice, c->stream));
    return 0;
  }
  const DType dt = t->f32 ? DT_F32 : c->dt;
  for (int s = 0; s < n; ++s)
    KCHK(launch_export_nchw(dt, t->p, out + (size_t)s * t->C * t->npos, t->C, t->npos, s * t->npos, t->ld, c->stream), "export support");
  return 0;
}

// The one-box-per-image form: the ROI list with roi_image[r] = r in B / shots segments of `shots` rows each.
int sylph_codegen_classes(sylph_ctx* c, const float* boxes, int shots, float* codes_out) {
  RET(refuse_on_record(c, "sylph_codegen_classes"));
  Plan* P = c->cur;
  if (!P) return fail("no current batch");
  if (!boxes || !codes_out) return fail("NULL argument");
  if (shots < 1 || P->B % shots != 0) return fail("pooled_features.shape[0] " + std::to_string(P->B) + " Vs batch_size * num_shots: the batch is not a whole number of classes");
  // a policy of this entry, not a limit of the kernels behind it (a segment of sylph_codegen_rois may be longer)
  if (shots > 64) return fail("codegen: " + std::to_string(shots) + " shots per class in one call; the shot reduction handles at most 64 (chunk the class and reduce the chunk codes, sylph_reduce_codes)");
  const std::vector<int> roi_image = identity_images(P->B), seg_len(P->B / shots, shots);
  return run_support(c, P, P->B, boxes, roi_image.data(), (int)seg_len.size(), seg_len.data(), codes_out, "codegen");
}

int sylph_codegen_rois(sylph_ctx* c, int R, const float* boxes, const int* roi_image, int n_seg, const int* seg_len, float* codes_out) {
  RET(refuse_on_record(c, "sylph_codegen_rois"));
  Plan* P = c->cur;
  RET(check_rois(P, R, boxes, roi_image));
  if (!seg_len || !codes_out) return fail("NULL argument");
  if (n_seg < 1) return fail("ROI list: n_seg = " + std::to_string(n_seg) + " (at least one segment is needed)");
  long total = 0;
  for (int j = 0; j < n_seg; ++j) {
    if (seg_len[j] < 1) return fail("ROI list: seg_len[" + std::to_string(j) + "] = " + std::to_string(seg_len[j]) + " (a segment needs at least one ROI)");
    total += seg_len[j];
  }
  if (total != R) return fail("ROI list: the segment lengths sum to " + std::to_string(total) + ", not to R = " + std::to_string(R));
  if (R > 65535) return fail("ROI list: R = " + std::to_string(R) + " ROIs in one call; at most 65535");
  return run_support(c, P, R, boxes, roi_image, n_seg, seg_len, codes_out, "codegen_rois");
}

/* see include/sylph_hip.h */
int sylph_shot_row_floats(sylph_ctx* c, int* n) {
  if (!n) return fail("NULL argument");
  if (c->cfg.cg_type != 1 && c->cfg.cg_code_ksize != 1 && c->cfg.cg_code_ksize != 3)
    return fail("sylph_shot_row_floats: cg_code_ksize " + std::to_string(c->cfg.cg_code_ksize) + " (1 or 3)");
  *n = shot_row_floats(c);
  return 0;
}

int sylph_codegen_shots(sylph_ctx* c, int R, const float* boxes, const int* roi_image, float* rows_out) {
  RET(refuse_on_record(c, "sylph_codegen_shots"));
  Plan* P = c->cur;
  RET(check_rois(P, R, boxes, roi_image));
  if (!rows_out) return fail("NULL argument");
  if (R > 65535) return fail("ROI list: R = " + std::to_string(R) + " ROIs in one call; at most 65535");
  return run_shots(c, P, R, boxes, roi_image, rows_out);
}

int sylph_shot_combine(sylph_ctx* c, const float* rows, int n_rows, int M, const int* idx, int n_seg, const int* seg_len, float* codes_out,
                       float* weight_norm_out) {
  const bool roienc = c->cfg.cg_type == 1;
  if (roienc ? !c->has_roienc : !c->has_codegen) return fail(roienc ? "ROIEncoder weights were not loaded" : "code generator weights were not loaded");
  if (!rows || !idx || !seg_len || !codes_out) return fail("NULL argument");
  if (n_rows < 1) return fail("shot bank: n_rows = " + std::to_string(n_rows) + " (the bank is empty)");
  if (M < 1) return fail("shot bank: M = " + std::to_string(M) + " (at least one index is needed)");
  if (n_seg < 1) return fail("shot bank: n_seg = " + std::to_string(n_seg) + " (at least one segment is needed)");
  for (int i = 0; i < M; ++i)
    if (idx[i] < 0 || idx[i] >= n_rows)
      return fail("shot bank: idx[" + std::to_string(i) + "] = " + std::to_string(idx[i]) + " is outside the bank of " + std::to_string(n_rows) + " rows");
  long total = 0;
  int max_len = 0;
  for (int j = 0; j < n_seg; ++j) {
    if (seg_len[j] < 1) return fail("shot bank: seg_len[" + std::to_string(j) + "] = " + std::to_string(seg_len[j]) + " (a segment needs at least one shot)");
    if (seg_len[j] > TAIL_MAX_LEN)
      return fail("shot bank: seg_len[" + std::to_string(j) + "] = " + std::to_string(seg_len[j]) + " shots in one segment; at most " + std::to_string(TAIL_MAX_LEN));
    total += seg_len[j];
    max_len = seg_len[j] > max_len ? seg_len[j] : max_len;
  }
  if (total != M) return fail("shot bank: the segment lengths sum to " + std::to_string(total) + ", not to M = " + std::to_string(M));
  HIPCHK(hipSetDevice(c->device));
  // tables: idx [M] | {first index, shots} [n_seg], 8-byte aligned
  const size_t seg_off = ((size_t)M + 1) / 2 * 2, ints = seg_off + 2 * (size_t)n_seg, need = ints * sizeof(int);
  if (c->shot_ev) HIPCHK(hipEventSynchronize(c->shot_ev));
  else HIPCHK(hipEventCreateWithFlags(&c->shot_ev, hipEventDisableTiming));
  if (need > c->shot_tab_cap) {
    if (c->shot_tab) c->dfree(c->shot_tab);
    c->shot_tab = nullptr; c->shot_tab_cap = 0;
    RET(ctx_alloc(c, &c->shot_tab, need * 2));
    c->shot_tab_cap = need * 2;
  }
  const int hdim = c->cfg.head_fc_dim > 256 ? c->cfg.head_fc_dim : 256;
  if (roienc && n_seg > c->shot_seg_cap) {
    if (c->shot_cls) c->dfree(c->shot_cls);
    if (c->shot_h) c->dfree(c->shot_h);
    c->shot_cls = c->shot_h = nullptr; c->shot_seg_cap = 0;
    RET(ctx_alloc(c, (void**)&c->shot_cls, (size_t)n_seg * 2 * 256 * sizeof(float)));
    RET(ctx_alloc(c, (void**)&c->shot_h, (size_t)2 * n_seg * 2 * hdim * sizeof(float)));
    c->shot_seg_cap = n_seg * 2;
  }
  c->shot_host.assign(ints, 0);
  std::copy(idx, idx + M, c->shot_host.begin());
  for (int j = 0, i0 = 0; j < n_seg; i0 += seg_len[j], ++j) {
    c->shot_host[seg_off + 2 * j] = i0;
    c->shot_host[seg_off + 2 * j + 1] = seg_len[j];
  }
  HIPCHK(hipMemcpyAsync(c->shot_tab, c->shot_host.data(), need, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipEventRecord(c->shot_ev, c->stream));
  const int* idx_dev = reinterpret_cast<const int*>(c->shot_tab);
  const int2* seg_dev = reinterpret_cast<const int2*>(idx_dev + seg_off);
  const int row = shot_row_floats(c);
  if (roienc) {
    KCHK(launch_shot_mean_tokens(rows, row, idx_dev, seg_dev, n_seg, c->shot_cls, c->stream), "shot_combine (token mean)");
    KCHK(launch_roienc_heads(c, c->shot_cls, n_seg, c->shot_h, c->shot_seg_cap, hdim, codes_out, c->stream), "shot_combine (heads)");
    return 0;
  }
  KCHK(launch_shot_combine(rows, row, idx_dev, seg_dev, n_seg, max_len, row - 4, c->cg_ib >= 0, c->cg_iw >= 0, c->cg_is >= 0, codes_out,
                           weight_norm_out, c->stream),
       "shot_combine");
  return 0;
}

int sylph_roi_table_uploads(sylph_ctx* c, int64_t* n) {
  if (!n) return fail("NULL argument");
  *n = c->roi_table_uploads;
  return 0;
}

int sylph_codegen_weight_norm(sylph_ctx* c, float* out) {
  Plan* P = c->cur;
  const SupportPass* Q = P ? P->sup_last : nullptr;
  if (!Q || !Q->built || !Q->cg_wnorm) return fail("no code-generator pass on the current batch");
  if (!c->cfg.cg_has_scale) return fail("CODE_GENERATOR.SCALE_LAYER is empty: there is no cls_weight_norm");
  HIPCHK(hipMemcpyAsync(out, Q->cg_wnorm, (size_t)Q->n_seg * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  return 0;
}

int sylph_codegen(sylph_ctx* c, const float* boxes, float* code_out) {
  RET(refuse_on_record(c, "sylph_codegen"));
  if (!c->cur) return fail("no current batch");
  return sylph_codegen_classes(c, boxes, c->cur->B, code_out);
}

int sylph_normalize_codes(sylph_ctx* c, float* codes, int n, const float* weight_norm) {
  if (!c->has_codegen) return fail("code generator weights were not loaded");
  if (n <= 0) return 0;
  const float prior = c->cg_bias_prior;
  KCHK(launch_normalize_codes(codes, n, 256, c->cfg.cg_code_ksize, c->cg_post.gamma, c->cg_post.beta, c->cfg.cg_post_norm,
                              c->cfg.cg_conv_l2_norm, c->cg_conv_scale, c->cg_bias_scale, prior, weight_norm, c->stream),
       "normalize_codes");
  return 0;
}

int sylph_reduce_codes(sylph_ctx* c, const float* rows, int n, int row_ld, float* out, int num_classes, int divide_by_acc) {
  if (!rows || !out) return fail("NULL argument");
  if (c->cfg.cg_code_ksize != 1)
    return fail("sylph_reduce_codes: the packed rows hold 1x1 class codes only (CODE_GENERATOR.CLS_LAYER kernel size 3 is not supported here)");
  if (row_ld < 262) return fail("sylph_reduce_codes: rows must be at least 262 floats wide");
  if (num_classes <= 0 || n < 0) return fail("sylph_reduce_codes: bad sizes");
  HIPCHK(hipSetDevice(c->device));
  KCHK(launch_reduce_codes(rows, n, row_ld, out, num_classes, divide_by_acc, c->stream), "reduce_codes");
  return 0;
}

}  // extern "C"
