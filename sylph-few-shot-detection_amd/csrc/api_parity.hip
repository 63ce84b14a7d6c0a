// Host side of libsylph_hip.so, unit "parity": single-kernel / single-block parity and micro-benchmark entries used by tests/ and tools/.
// No torch types, no CPU compute fallback: every stage is a HIP kernel from this directory.
#include "api_internal.h"

namespace {

// B images between the caller's fp32 NCHW tensors and dense device images [B][hw][C] of the context's storage type
int import_nchw(sylph_ctx* c, const float* src, void* dst, int B, int C, int hw, const char* what = "import") {
  for (int b = 0; b < B; ++b) KCHK(launch_import_nchw(c->dt, src + (size_t)b * C * hw, dst, C, hw, b * hw, C, c->stream), what);
  return 0;
}
int export_nchw(sylph_ctx* c, const void* src, float* dst, int B, int C, int hw, const char* what = "export") {
  for (int b = 0; b < B; ++b) KCHK(launch_export_nchw(c->dt, src, dst + (size_t)b * C * hw, C, hw, b * hw, C, c->stream), what);
  return 0;
}

// The scratch context of one parity entry: the builders allocate, upload and record into it as into any context, it works on the caller's
// device, stream, storage type, zero page and configuration, and on return it drains the stream and frees what it allocated.
//   Records::to_caller  profiling follows the caller's, and hand_records() moves the profile + route records of the entry's launches to the
//                       caller's context (conv2d, bottleneck*, group_conv, conv3x3_c64, basic_block, fpn_lateral)
//   Records::none       the entry's launches are never profiled (group_norm, stem_maxpool, bench_conv)
enum class Records { to_caller, none };
struct Scratch : sylph_ctx {
  sylph_ctx* const caller;
  Scratch(sylph_ctx* c, Records rec) : caller(c) {
    device = c->device; dt = c->dt; stream = c->stream; zeros = c->zeros; cfg = c->cfg;
    if (rec == Records::to_caller) prof = c->prof;
  }
  Scratch(const Scratch&) = delete;
  ~Scratch() {
    (void)hipStreamSynchronize(stream);
    for (void* p : allocs) (void)hipFree(p);
  }
  void hand_records() { adopt_records(caller, this); }
};

}  // namespace

extern "C" {

int sylph_conv2d(sylph_ctx* c, const float* x, int B, int C, int H, int W, const float* w_host, int Cout, int KH, int KW,
                 int stride, int pad, const float* scale_host, const float* shift_host, int relu, const float* residual,
                 float* y) {
  HIPCHK(hipSetDevice(c->device));
  const int bk = c->dt == DT_BF16 ? 64 : 32;
  if (C % bk != 0) return fail("sylph_conv2d: Cin must be a multiple of " + std::to_string(bk));
  const int Ho = (H + 2 * pad - KH) / stride + 1, Wo = (W + 2 * pad - KW) / stride + 1;
  Scratch tmp(c, Records::to_caller);
  HostTensor hw;
  hw.shape = {Cout, C, KH, KW};
  hw.data.assign(w_host, w_host + (size_t)Cout * C * KH * KW);
  ConvLayer L;
  RET(pack_conv(&tmp, {&hw}, &L));
  if (scale_host) RET(upload_vec(&tmp, &L.scale, std::vector<float>(scale_host, scale_host + Cout), L.Cout_pad));
  if (shift_host) RET(upload_vec(&tmp, &L.shift, std::vector<float>(shift_host, shift_host + Cout), L.Cout_pad));
  void *xin, *yout, *res = nullptr;
  RET(tmp.dalloc(&xin, (size_t)B * H * W * C * tmp.esz()));
  RET(tmp.dalloc(&yout, (size_t)B * Ho * Wo * Cout * tmp.esz()));
  RET(import_nchw(&tmp, x, xin, B, C, H * W));
  ConvOpts o; o.stride = stride; o.pad = pad; o.relu_nch = relu ? (1 << 30) : 0;
  if (residual) {
    RET(tmp.dalloc(&res, (size_t)B * Ho * Wo * Cout * tmp.esz()));
    RET(import_nchw(&tmp, residual, res, B, Cout, Ho * Wo));
    o.res = res; o.res_ld = Cout; o.res_mode = 1;
  }
  std::vector<OpFn> ops;
  RET(add_conv(&tmp, ops, L, xin, C, yout, Cout, image_segs(B, H, W, Ho, Wo), o));
  RET(run_ops(c, ops, "conv2d"));
  tmp.hand_records();
  return export_nchw(&tmp, yout, y, B, Cout, Ho * Wo);
}

int sylph_set_debug_taps(sylph_ctx* c, int on) {
  c->debug_taps = on != 0;
  return 0;
}

int sylph_export_stage(sylph_ctx* c, int stage, float* out) {
  RET(refuse_on_record(c, "sylph_export_stage"));
  Plan* P = c->cur;
  if (!P || !P->backbone_built) return fail("no backbone pass on the current batch");
  const bool on_demand = stage == 2 && P->tail_even;
  if (stage < 2 || stage > 5 || (!P->stage_out[stage - 2] && !on_demand)) return fail("bad stage");
  HIPCHK(hipSetDevice(c->device));
  const int si = stage - 2, C = P->stage_c[si], hw = P->stage_h[si] * P->stage_w[si];
  const void* src = P->stage_out[si];
  if (on_demand) {
    // the step computed res2 at the positions res3 reads only: run the last block's DENSE launch now, from its input (intact in the stage's
    // other ping-pong buffer) into a buffer of the tap's own.  Nothing the step or a later head / decode reads is written.
    if (!P->tail_dense) {
      OwnerScope own(c, P);
      RET(c->dalloc(&P->tail_dense, (size_t)P->B * hw * C * c->esz()));
      BkScratch scr{nullptr, nullptr, nullptr, &P->bk_trash};
      const int rc = add_bottleneck(c, P->tail_dense_ops, c->stages[0].back(), P->B, P->tail_x, C, P->stage_h[si], P->stage_w[si], 1, 64, C, P->tail_dense, scr);
      if (rc != 0) { P->tail_dense_ops.clear(); return rc; }
    }
    RET(run_ops(c, P->tail_dense_ops, "res2 tap"));
    src = P->tail_dense;
  }
  if (const int ld = P->stage_ld[si]; ld && ld != C) {  // (MobileNetV2: rows of ld stored channels, the first C are the stage's)
    for (int b = 0; b < P->B; ++b) KCHK(launch_export_nchw(c->dt, src, out + (size_t)b * C * hw, C, hw, b * hw, ld, c->stream), "export stage");
    return 0;
  }
  return export_nchw(c, src, out, P->B, C, hw, "export stage");
}

int sylph_export_tower(sylph_ctx* c, int tower, int layer, int level, float* y, float* coef) {
  RET(refuse_on_record(c, "sylph_export_tower"));
  Plan* P = c->cur;
  if (!P || !P->head_built) return fail("no head pass on the current batch");
  if (tower < 0 || tower > 1 || layer < 0 || layer >= (int)P->tap_out[tower].size()) return fail("bad tower / layer");
  if (level < 0 || level >= c->cfg.nlevels) return fail("bad level");
  if (!c->debug_taps && layer + 1 != (int)P->tap_out[tower].size()) return fail("intermediate tower layers need sylph_set_debug_taps(1) before the first head call");
  HIPCHK(hipSetDevice(c->device));
  const int hw = P->hl[level] * P->wl[level], L = c->cfg.nlevels;
  for (int b = 0; b < P->B; ++b) {
    if (y) KCHK(launch_export_nchw(c->dt, P->tap_out[tower][layer], y + (size_t)b * 256 * hw, 256, hw, b * P->Ltot + P->off[level], 256, c->stream), "export tower");
    if (coef) {
      if (!P->tap_coef[tower][layer]) return fail("this layer's GroupNorm was applied in place (no coefficient table)");
      HIPCHK(hipMemcpyAsync(coef + (size_t)b * 512, P->tap_coef[tower][layer] + (size_t)(b * L + level) * 256, 512 * sizeof(float),
                            hipMemcpyDeviceToDevice, c->stream));
    }
  }
  return 0;
}

// even_out: the stride-2-output launch of the fused identity block (BK_EVEN_OUT), y (B, cout, H/2, W/2)
static int bottleneck_entry(sylph_ctx* c, const float* x, int B, int Cin, int H, int W, int stride, int mid, int cout, int groups,
                            const float* const* w_host, const float* const* scale_host, const float* const* shift_host, float* y, bool even_out = false) {
  HIPCHK(hipSetDevice(c->device));
  const int bk = c->dt == DT_BF16 ? 64 : 32;
  if (Cin % bk != 0 || mid % bk != 0) return fail("sylph_bottleneck: channel counts must be multiples of " + std::to_string(bk));
  const bool has_sc = w_host[3] != nullptr;
  if (!has_sc && (Cin != cout || stride != 1)) return fail("sylph_bottleneck: an identity block needs Cin == cout and stride 1");
  Scratch tmp(c, Records::to_caller);
  sylph_ctx::Block blk;
  const int cins[4] = {Cin, mid, mid, Cin}, couts[4] = {mid, mid, cout, cout}, ks[4] = {1, 3, 1, 1};
  ConvLayer* Ls[4] = {&blk.c1, &blk.c2, &blk.c3, &blk.sc};
  HostTensor hw[4];
  for (int i = 0; i < (has_sc ? 4 : 3); ++i) {
    const int cin_w = i == 1 ? cins[i] / groups : cins[i];
    hw[i].shape = {couts[i], cin_w, ks[i], ks[i]};
    hw[i].data.assign(w_host[i], w_host[i] + (size_t)couts[i] * cin_w * ks[i] * ks[i]);
    if (i == 1 && groups > 1) {  // ResNeXt conv2 (conv_group.hip)
      RET(pack_conv_grouped(&tmp, hw[i], "conv2.weight", mid, groups, scale_host[i], shift_host[i], Ls[i]));
      continue;
    }
    RET(pack_conv(&tmp, {&hw[i]}, Ls[i]));
    RET(upload_vec(&tmp, &Ls[i]->scale, std::vector<float>(scale_host[i], scale_host[i] + couts[i]), Ls[i]->Cout_pad));
    RET(upload_vec(&tmp, &Ls[i]->shift, std::vector<float>(shift_host[i], shift_host[i] + couts[i]), Ls[i]->Cout_pad));
  }
  blk.has_sc = has_sc;
  if (has_sc && knob::fuse_shortcut()) {
    RET(make_c3sc(&tmp, hw[2], scale_host[2], shift_host[2], hw[3], scale_host[3], shift_host[3], &blk.c3sc));
    blk.fused_sc = true;
  }
  const size_t e = tmp.esz();
  const int Ho = even_out ? H / 2 : (H - 1) / stride + 1, Wo = even_out ? W / 2 : (W - 1) / stride + 1;
  void *xin, *yout, *t1, *t2, *sc, *trash = nullptr;
  RET(tmp.dalloc(&xin, (size_t)B * H * W * Cin * e));
  RET(tmp.dalloc(&yout, (size_t)B * Ho * Wo * cout * e));
  RET(tmp.dalloc(&t1, (size_t)B * H * W * mid * e));
  RET(tmp.dalloc(&t2, (size_t)B * Ho * Wo * mid * e));
  RET(tmp.dalloc(&sc, (size_t)B * Ho * Wo * cout * e));
  RET(import_nchw(&tmp, x, xin, B, Cin, H * W));
  std::vector<OpFn> ops;
  BkScratch scr{t1, t2, sc, &trash};
  RET(add_bottleneck(&tmp, ops, blk, B, xin, Cin, H, W, stride, mid, cout, yout, scr, even_out ? BK_EVEN_OUT : 0));
  RET(run_ops(c, ops, "bottleneck"));
  tmp.hand_records();
  return export_nchw(&tmp, yout, y, B, cout, Ho * Wo);
}

int sylph_bottleneck(sylph_ctx* c, const float* x, int B, int Cin, int H, int W, int stride, int mid, int cout, const float* const* w_host,
                     const float* const* scale_host, const float* const* shift_host, float* y) {
  return bottleneck_entry(c, x, B, Cin, H, W, stride, mid, cout, 1, w_host, scale_host, shift_host, y);
}

int sylph_bottleneck_even(sylph_ctx* c, const float* x, int B, int Cin, int H, int W, int mid, int cout, const float* const* w_host,
                          const float* const* scale_host, const float* const* shift_host, float* y) {
  if (B < 1 || H < 2 || W < 2 || (H & 1) || (W & 1)) return fail("sylph_bottleneck_even: H and W must be even");
  if (Cin != 256 || mid != 64 || cout != 256 || c->dt != DT_BF16) return fail("sylph_bottleneck_even: the fused identity block is C 256, mid 64, bf16");
  if (!w_host[0] || !w_host[1] || !w_host[2] || w_host[3]) return fail("sylph_bottleneck_even: an identity block has three convs and no shortcut");
  return bottleneck_entry(c, x, B, Cin, H, W, 1, mid, cout, 1, w_host, scale_host, shift_host, y, true);
}

// The res3 block-pair launch alone (conv_spw_pair.hip): t2 (B, 128, H, W), x (B, 512, H, W) ->
// y = relu(bn3(w3 t2) + x) (B, 512, H, W) and t1 = relu(bn1(w1 y)) (B, 128, H, W); w3 (512, 128), w1 (128, 512)
int sylph_res3_pair(sylph_ctx* c, const float* t2, const float* x, int B, int H, int W, const float* w3_host, const float* s3_host,
                    const float* b3_host, const float* w1_host, const float* s1_host, const float* b1_host, float* y, float* t1) {
  HIPCHK(hipSetDevice(c->device));
  if (c->dt != DT_BF16) return fail("sylph_res3_pair: the pair kernel is bf16");
  if (B < 1 || H < 1 || W < 1 || (long)H * W * 1024 >= (1L << 32) || (long)B * H * W >= (1L << 31)) return fail("sylph_res3_pair: bad shape");
  if (!t2 || !x || !w3_host || !s3_host || !b3_host || !w1_host || !s1_host || !b1_host || !y || !t1) return fail("sylph_res3_pair: null argument");
  Scratch tmp(c, Records::to_caller);
  HostTensor h3, h1;
  h3.shape = {512, 128, 1, 1}; h3.data.assign(w3_host, w3_host + (size_t)512 * 128);
  h1.shape = {128, 512, 1, 1}; h1.data.assign(w1_host, w1_host + (size_t)128 * 512);
  ConvLayer L3, L1;
  RET(pack_conv(&tmp, {&h3}, &L3));
  RET(pack_conv(&tmp, {&h1}, &L1));
  if (L3.Cout_pad != 512 || L1.Cout_pad != 128) return fail("internal: sylph_res3_pair weight padding");
  RET(upload_vec(&tmp, &L3.scale, std::vector<float>(s3_host, s3_host + 512), 512));
  RET(upload_vec(&tmp, &L3.shift, std::vector<float>(b3_host, b3_host + 512), 512));
  RET(upload_vec(&tmp, &L1.scale, std::vector<float>(s1_host, s1_host + 128), 128));
  RET(upload_vec(&tmp, &L1.shift, std::vector<float>(b1_host, b1_host + 128), 128));
  const size_t hw = (size_t)H * W, e = tmp.esz();
  void *t2d, *xd, *yd, *t1d;
  RET(tmp.dalloc(&t2d, B * hw * 128 * e));
  RET(tmp.dalloc(&xd, B * hw * 512 * e));
  RET(tmp.dalloc(&yd, B * hw * 512 * e));
  RET(tmp.dalloc(&t1d, B * hw * 128 * e));
  RET(import_nchw(&tmp, t2, t2d, B, 128, (int)hw));
  RET(import_nchw(&tmp, x, xd, B, 512, (int)hw));
  std::vector<OpFn> ops;
  RET(add_res3_pair(&tmp, ops, L3, L1, B, (int)hw, t2d, xd, yd, t1d));
  RET(run_ops(c, ops, "res3_pair"));
  tmp.hand_records();
  RET(export_nchw(&tmp, yd, y, B, 512, (int)hw));
  return export_nchw(&tmp, t1d, t1, B, 128, (int)hw);
}

int sylph_bottleneck_grouped(sylph_ctx* c, const float* x, int B, int Cin, int H, int W, int stride, int mid, int cout, int groups,
                             const float* const* w_host, const float* const* scale_host, const float* const* shift_host, float* y) {
  if (groups < 1 || mid % groups != 0) return fail("sylph_bottleneck_grouped: mid must be a multiple of groups");
  return bottleneck_entry(c, x, B, Cin, H, W, stride, mid, cout, groups, w_host, scale_host, shift_host, y);
}

int sylph_group_conv(sylph_ctx* c, const float* x, int B, int C, int H, int W, int groups, int stride, const float* w_host,
                     const float* scale_host, const float* shift_host, int relu, float* y) {
  HIPCHK(hipSetDevice(c->device));
  if (groups < 1 || C % groups != 0 || (stride != 1 && stride != 2) || B < 1) return fail("sylph_group_conv: bad arguments");
  Scratch tmp(c, Records::to_caller);
  HostTensor hw;
  hw.shape = {C, C / groups, 3, 3};
  hw.data.assign(w_host, w_host + (size_t)C * (C / groups) * 9);
  ConvLayer L;
  RET(pack_conv_grouped(&tmp, hw, "sylph_group_conv weight", C, groups, scale_host, shift_host, &L));
  const size_t e = tmp.esz();
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  void *xin, *yout;
  RET(tmp.dalloc(&xin, (size_t)B * H * W * C * e));
  RET(tmp.dalloc(&yout, (size_t)B * Ho * Wo * C * e));
  RET(import_nchw(&tmp, x, xin, B, C, H * W));
  GroupConvArgs ga;
  memset(&ga, 0, sizeof(ga));
  ga.x = xin; ga.y = yout; ga.wt = L.w; ga.scale = L.scale; ga.shift = L.shift;
  ga.B = B; ga.C = C; ga.cpg = C / groups; ga.Hin = H; ga.Win = W; ga.Ho = Ho; ga.Wo = Wo; ga.stride = stride; ga.relu = relu ? 1 : 0;
  const double fl = 2.0 * (double)B * Ho * Wo * C * 9.0 * (C / groups);
  const DType dt = c->dt;
  KCHK(timed_op(&tmp, "conv_group_kernel", fl, c->stream, [=](hipStream_t st) { return launch_conv_group(dt, ga, st); }), "conv_group");
  tmp.hand_records();
  return export_nchw(&tmp, yout, y, B, C, Ho * Wo);
}

int sylph_conv3x3_c64(sylph_ctx* c, const float* x, int B, int H, int W, const float* w_host, const float* scale_host,
                      const float* shift_host, int relu, const float* residual, float* y) {
  HIPCHK(hipSetDevice(c->device));
  if (B < 1 || H < 1 || W < 1 || !w_host || !scale_host || !shift_host) return fail("sylph_conv3x3_c64: bad arguments");
  Scratch tmp(c, Records::to_caller);
  HostTensor hw;
  hw.shape = {64, 64, 3, 3};
  hw.data.assign(w_host, w_host + (size_t)64 * 64 * 9);
  ConvLayer L;
  RET(pack_conv(&tmp, {&hw}, &L));
  RET(upload_vec(&tmp, &L.scale, std::vector<float>(scale_host, scale_host + 64), L.Cout_pad));
  RET(upload_vec(&tmp, &L.shift, std::vector<float>(shift_host, shift_host + 64), L.Cout_pad));
  const size_t n = (size_t)B * H * W * 64 * tmp.esz();
  void *xin, *yout, *res = nullptr;
  RET(tmp.dalloc(&xin, n));
  RET(tmp.dalloc(&yout, n));
  if (residual) RET(tmp.dalloc(&res, n));
  RET(import_nchw(&tmp, x, xin, B, 64, H * W));
  if (residual) RET(import_nchw(&tmp, residual, res, B, 64, H * W));
  std::vector<OpFn> ops;
  RET(add_conv3x3_c64(&tmp, ops, L, B, H, W, xin, res, yout, relu));
  RET(run_ops(c, ops, "conv3x3_c64"));
  tmp.hand_records();
  return export_nchw(&tmp, yout, y, B, 64, H * W);
}

int sylph_basic_block(sylph_ctx* c, const float* x, int B, int Cin, int H, int W, int stride, int cout, const float* const* w_host,
                      const float* const* scale_host, const float* const* shift_host, float* y) {
  HIPCHK(hipSetDevice(c->device));
  const int bk = c->dt == DT_BF16 ? 64 : 32;
  if (Cin % bk != 0 || cout % bk != 0) return fail("sylph_basic_block: channel counts must be multiples of " + std::to_string(bk));
  if (stride != 1 && stride != 2) return fail("sylph_basic_block: stride must be 1 or 2");
  const bool has_sc = w_host[2] != nullptr;
  if (!has_sc && (Cin != cout || stride != 1)) return fail("sylph_basic_block: an identity block needs Cin == cout and stride 1");
  Scratch tmp(c, Records::to_caller);
  sylph_ctx::Block blk;
  blk.basic = true; blk.has_sc = has_sc;
  const int cins[3] = {Cin, cout, Cin}, ks[3] = {3, 3, 1};
  ConvLayer* Ls[3] = {&blk.c1, &blk.c2, &blk.sc};
  HostTensor hw[3];
  for (int i = 0; i < (has_sc ? 3 : 2); ++i) {
    hw[i].shape = {cout, cins[i], ks[i], ks[i]};
    hw[i].data.assign(w_host[i], w_host[i] + (size_t)cout * cins[i] * ks[i] * ks[i]);
    RET(pack_conv(&tmp, {&hw[i]}, Ls[i]));
    RET(upload_vec(&tmp, &Ls[i]->scale, std::vector<float>(scale_host[i], scale_host[i] + cout), Ls[i]->Cout_pad));
    RET(upload_vec(&tmp, &Ls[i]->shift, std::vector<float>(shift_host[i], shift_host[i] + cout), Ls[i]->Cout_pad));
  }
  const size_t e = tmp.esz();
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  void *xin, *yout, *t1, *sc, *trash = nullptr;
  RET(tmp.dalloc(&xin, (size_t)B * H * W * Cin * e));
  RET(tmp.dalloc(&yout, (size_t)B * Ho * Wo * cout * e));
  RET(tmp.dalloc(&t1, (size_t)B * Ho * Wo * cout * e));
  RET(tmp.dalloc(&sc, (size_t)B * Ho * Wo * cout * e));
  RET(import_nchw(&tmp, x, xin, B, Cin, H * W));
  std::vector<OpFn> ops;
  BkScratch scr{t1, nullptr, sc, &trash};
  RET(add_basic_block(&tmp, ops, blk, B, xin, Cin, H, W, stride, cout, yout, scr));
  RET(run_ops(c, ops, "basic_block"));
  tmp.hand_records();
  return export_nchw(&tmp, yout, y, B, cout, Ho * Wo);
}

int sylph_mbv2_padded_channels(sylph_ctx* c, int C) { return mbv2_pad(c, C); }

int sylph_dwconv3x3(sylph_ctx* c, const float* x, int B, int C, int H, int W, int stride, const float* w_host, const float* scale_host,
                    const float* shift_host, float* y) {
  HIPCHK(hipSetDevice(c->device));
  if (B < 1 || C < 8 || (C & 7) || H < 1 || W < 1 || (stride != 1 && stride != 2) || !x || !w_host || !scale_host || !shift_host || !y)
    return fail("sylph_dwconv3x3: bad arguments (C a multiple of 8, stride 1 or 2)");
  Scratch tmp(c, Records::to_caller);
  HostTensor hw;
  hw.shape = {C, 1, 3, 3};
  hw.data.assign(w_host, w_host + (size_t)C * 9);
  float *wd, *sd, *hd;
  RET(make_dw_table(&tmp, hw, C, C, scale_host, shift_host, &wd, &sd, &hd));
  const size_t e = tmp.esz();
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  void *xin, *yout;
  RET(tmp.dalloc(&xin, (size_t)B * H * W * C * e));
  RET(tmp.dalloc(&yout, (size_t)B * Ho * Wo * C * e));
  RET(import_nchw(&tmp, x, xin, B, C, H * W));
  std::vector<OpFn> ops;
  RET(add_dwconv3x3(&tmp, ops, wd, sd, hd, B, C, C, H, W, stride, xin, yout));
  RET(run_ops(c, ops, "dwconv3x3"));
  tmp.hand_records();
  return export_nchw(&tmp, yout, y, B, C, Ho * Wo);
}

int sylph_mbv2_block(sylph_ctx* c, const float* x, int B, int Cin, int H, int W, int t, int Cout, int stride, const float* const* w_host,
                     const float* const* scale_host, const float* const* shift_host, int y_channels, float* y) {
  HIPCHK(hipSetDevice(c->device));
  if (B < 1 || Cin < 1 || Cout < 1 || H < 1 || W < 1 || (t != 1 && t != 6) || (stride != 1 && stride != 2) || !x || !y || !w_host || !scale_host || !shift_host)
    return fail("sylph_mbv2_block: bad arguments (t 1 or 6, stride 1 or 2)");
  if ((t != 1) != (w_host[0] != nullptr) || !w_host[1] || !w_host[2]) return fail("sylph_mbv2_block: an expand conv exactly when t != 1");
  for (int i = t != 1 ? 0 : 1; i < 3; ++i)
    if (!scale_host[i] || !shift_host[i]) return fail("sylph_mbv2_block: a FrozenBN scale and shift for every conv of the block");
  const int hid = Cin * t;
  Scratch tmp(c, Records::to_caller);
  HostTensor hw[3];
  const HostTensor* hp[3] = {nullptr, &hw[1], &hw[2]};
  if (t != 1) { hw[0].shape = {hid, Cin, 1, 1}; hw[0].data.assign(w_host[0], w_host[0] + (size_t)hid * Cin); hp[0] = &hw[0]; }
  hw[1].shape = {hid, 1, 3, 3}; hw[1].data.assign(w_host[1], w_host[1] + (size_t)hid * 9);
  hw[2].shape = {Cout, hid, 1, 1}; hw[2].data.assign(w_host[2], w_host[2] + (size_t)Cout * hid);
  sylph_ctx::MbBlock blk;
  RET(make_mbv2_block(&tmp, Cin, t, Cout, stride, hp, scale_host, shift_host, &blk));
  if (y_channels != Cout && y_channels != blk.cout_p) return fail("sylph_mbv2_block: y_channels must be Cout or its padded count");
  if (pick_mbv2_route(&tmp, blk, B, H, W) == Mbv2Route::chain) {  // an image the chain refuses: before the buffers are allocated
    int run = 0;
    RET(mbv2_chain_run(blk, B, H, W, &run));
  }
  const size_t e = tmp.esz();
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  const size_t n_x = (size_t)B * H * W * blk.cin_ld * e;
  void *xin, *yout, *h1, *h2;
  RET(tmp.dalloc(&xin, n_x));
  RET(tmp.dalloc(&yout, (size_t)B * Ho * Wo * blk.cout_ld * e));
  RET(tmp.dalloc(&h1, (size_t)B * H * W * blk.hid_ld * e));
  RET(tmp.dalloc(&h2, (size_t)B * Ho * Wo * blk.hid_ld * e));
  HIPCHK(hipMemsetAsync(xin, 0, n_x, c->stream));  // the pad channels of the input are zero, as every producer leaves them
  for (int b = 0; b < B; ++b) KCHK(launch_import_nchw(c->dt, x + (size_t)b * Cin * H * W, xin, Cin, H * W, b * H * W, blk.cin_ld, c->stream), "import");
  std::vector<OpFn> ops;
  RET(add_mbv2_block(&tmp, ops, blk, B, xin, H, W, yout, h1, h2));
  RET(run_ops(c, ops, "mbv2_block"));
  tmp.hand_records();
  for (int b = 0; b < B; ++b)
    KCHK(launch_export_nchw(c->dt, yout, y + (size_t)b * y_channels * Ho * Wo, y_channels, Ho * Wo, b * Ho * Wo, blk.cout_ld, c->stream), "export");
  return 0;
}

int sylph_fpn_lateral(sylph_ctx* c, const float* x, int B, int C, int H, int W, const float* w_host, const float* bias_host, const float* top,
                      float* y) {
  HIPCHK(hipSetDevice(c->device));
  const int bk = c->dt == DT_BF16 ? 64 : 32;
  if (C % bk != 0) return fail("sylph_fpn_lateral: Cin must be a multiple of " + std::to_string(bk));
  if (top && ((H & 1) || (W & 1))) return fail("sylph_fpn_lateral: the top-down input is half the size: H and W must be even");
  Scratch tmp(c, Records::to_caller);
  HostTensor hw;
  hw.shape = {256, C, 1, 1};
  hw.data.assign(w_host, w_host + (size_t)256 * C);
  ConvLayer L;
  RET(pack_conv(&tmp, {&hw}, &L));
  RET(upload_vec(&tmp, &L.shift, std::vector<float>(bias_host, bias_host + 256), L.Cout_pad));
  const size_t e = tmp.esz();
  void *xin, *yout, *tp = nullptr;
  RET(tmp.dalloc(&xin, (size_t)B * H * W * C * e));
  RET(tmp.dalloc(&yout, (size_t)B * H * W * 256 * e));
  RET(import_nchw(&tmp, x, xin, B, C, H * W));
  ConvOpts o;
  std::vector<SegDesc> segs = image_segs(B, H, W, H, W);
  if (top) {  // exactly the launch build_backbone makes for fpn_lateral3 / 4: residual = nearest 2x upsample of the level above
    const int h2 = H / 2, w2 = W / 2;
    RET(tmp.dalloc(&tp, (size_t)B * h2 * w2 * 256 * e));
    RET(import_nchw(&tmp, top, tp, B, 256, h2 * w2));
    o.res = tp; o.res_ld = 256; o.res_mode = 2;
    segs = image_segs(B, H, W, H, W, h2, w2);
  }
  std::vector<OpFn> ops;
  RET(add_conv(&tmp, ops, L, xin, C, yout, 256, segs, o));
  RET(run_ops(c, ops, "fpn_lateral"));
  tmp.hand_records();
  return export_nchw(&tmp, yout, y, B, 256, H * W);
}

int sylph_group_norm(sylph_ctx* c, const float* x, int B, int H, int W, const float* gamma_host, const float* beta_host,
                     int relu, float* y) {
  HIPCHK(hipSetDevice(c->device));
  Scratch tmp(c, Records::none);
  const int HW = H * W;
  void* buf;
  RET(tmp.dalloc(&buf, (size_t)B * HW * 256 * tmp.esz()));
  RET(import_nchw(&tmp, x, buf, B, 256, HW));
  std::vector<RowSeg> rs;
  for (int b = 0; b < B; ++b) rs.push_back(RowSeg{b * HW, HW});
  RowSeg* rsd;
  RET(upload(&tmp, (void**)&rsd, rs.data(), rs.size() * sizeof(RowSeg)));
  float *ga, *be, *partial;
  float2* stats;
  RET(upload_vec(&tmp, &ga, std::vector<float>(gamma_host, gamma_host + 256), 256));
  RET(upload_vec(&tmp, &be, std::vector<float>(beta_host, beta_host + 256), 256));
  const int max_chunks = (HW + GN_ROWS_PER_CHUNK - 1) / GN_ROWS_PER_CHUNK;
  RET(tmp.dalloc((void**)&partial, (size_t)B * max_chunks * 32 * 3 * 4));
  RET(tmp.dalloc((void**)&stats, (size_t)B * 32 * sizeof(float2)));
  KCHK(launch_groupnorm(c->dt, buf, rsd, B, HW, 256, ga, be, 1e-5f, relu, partial, stats, c->stream), "group_norm");
  return export_nchw(&tmp, buf, y, B, 256, HW);
}

int sylph_stem_maxpool(sylph_ctx* c, const float* x, int B, int H, int W, const float* w_host, const float* scale_host,
                       const float* shift_host, float* stem_out, float* pool_out) {
  if (c->dt != DT_BF16) return fail("sylph_stem_maxpool: the dedicated stem kernels exist in bf16 mode only");
  HIPCHK(hipSetDevice(c->device));
  Scratch tmp(c, Records::none);
  const int H2 = (H - 1) / 2 + 1, W2 = (W - 1) / 2 + 1, H4 = (H2 - 1) / 2 + 1, W4 = (W2 - 1) / 2 + 1;
  std::vector<bf16_t> wp((size_t)64 * 224);  // [n][kh][8 px][4 ch], kernel column 7 / channel 3 zero (as sylph_finalize_weights)
  for (int n = 0; n < 64; ++n)
    for (int kh = 0; kh < 7; ++kh)
      for (int px = 0; px < 8; ++px)
        for (int ch = 0; ch < 4; ++ch)
          wp[(size_t)n * 224 + kh * 32 + px * 4 + ch] = (bf16_t)((px < 7 && ch < 3) ? w_host[((n * 3 + ch) * 7 + kh) * 7 + px] : 0.f);
  void *wpd, *x0, *so, *po;
  float *scd, *shd;
  ImageDesc* idd;
  RET(upload(&tmp, &wpd, wp.data(), wp.size() * sizeof(bf16_t)));
  RET(upload_vec(&tmp, &scd, std::vector<float>(scale_host, scale_host + 64), 64));
  RET(upload_vec(&tmp, &shd, std::vector<float>(shift_host, shift_host + 64), 64));
  std::vector<ImageDesc> id((size_t)B);
  for (int b = 0; b < B; ++b) { id[b].ptr = x + (size_t)b * 3 * H * W; id[b].h = H; id[b].w = W; }
  RET(upload(&tmp, (void**)&idd, id.data(), id.size() * sizeof(ImageDesc)));
  RET(tmp.dalloc(&x0, (size_t)B * H * W * 4 * 2));
  RET(tmp.dalloc(&so, (size_t)B * H2 * W2 * 64 * 2));
  RET(tmp.dalloc(&po, (size_t)B * H4 * W4 * 64 * 2));
  const float mean0[3] = {0.f, 0.f, 0.f}, std1[3] = {1.f, 1.f, 1.f};
  KCHK(launch_preprocess(c->dt, idd, x0, B, H, W, mean0, std1, c->stream), "preprocess");
  KCHK(launch_stem_conv(x0, wpd, scd, shd, so, B, H, W, H2, W2, c->stream), "stem_conv");
  if (knob::fuse_stem_pool()) {  // the product path: pool_out comes from the fused kernel, stem_out from the stand-alone stem kernel
    void* trash;
    RET(tmp.dalloc(&trash, (size_t)512 * 256 * 16));
    KCHK(launch_stem_pool(x0, wpd, scd, shd, po, trash, B, H, W, H2, W2, H4, W4, c->stream), "stem_pool");
  } else {
    KCHK(launch_maxpool(c->dt, so, po, B, H2, W2, 64, H4, W4, c->stream), "maxpool");
  }
  if (stem_out) RET(export_nchw(&tmp, so, stem_out, B, 64, H2 * W2));
  if (pool_out) RET(export_nchw(&tmp, po, pool_out, B, 64, H4 * W4));
  return 0;
}

int sylph_bench_conv(sylph_ctx* c, int B, int H, int W, int Cin, int Cout, int K, int stride, int pad, int has_res,
                     int relu, int with_gn, int iters, float* ms_out, double* flops_out) {
  HIPCHK(hipSetDevice(c->device));
  const int bk = c->dt == DT_BF16 ? 64 : 32;
  if (Cin % bk != 0) return fail("sylph_bench_conv: Cin must be a multiple of " + std::to_string(bk));
  const int Ho = (H + 2 * pad - K) / stride + 1, Wo = (W + 2 * pad - K) / stride + 1;
  Scratch tmp(c, Records::none);
  HostTensor hw;
  hw.shape = {Cout, Cin, K, K};
  hw.data.resize((size_t)Cout * Cin * K * K);
  unsigned st = 12345u;
  const float wsc = 1.0f / sqrtf((float)(Cin * K * K));
  for (auto& v : hw.data) { st = st * 1664525u + 1013904223u; v = ((float)(st >> 8) * (2.0f / 16777216.0f) - 1.0f) * wsc; }
  ConvLayer L;
  RET(pack_conv(&tmp, {&hw}, &L));
  RET(upload_vec(&tmp, &L.scale, std::vector<float>((size_t)Cout, 1.0f), L.Cout_pad));
  RET(upload_vec(&tmp, &L.shift, std::vector<float>((size_t)Cout, 0.1f), L.Cout_pad));
  void *xin, *yout, *res = nullptr;
  const size_t nin = (size_t)B * H * W * Cin, nout = (size_t)B * Ho * Wo * Cout;
  RET(tmp.dalloc(&xin, nin * tmp.esz()));
  RET(tmp.dalloc(&yout, nout * tmp.esz()));
  KCHK(launch_fill_random(c->dt, xin, nin, 1u, c->stream), "fill");
  ConvOpts o; o.stride = stride; o.pad = pad; o.relu_nch = relu ? (1 << 30) : 0;
  if (has_res) {
    RET(tmp.dalloc(&res, nout * tmp.esz()));
    KCHK(launch_fill_random(c->dt, res, nout, 2u, c->stream), "fill");
    o.res = res; o.res_ld = Cout; o.res_mode = 1;
  }
  o.want_gn = with_gn & 1;
  if (with_gn & 2) {  // fused GroupNorm + ReLU of the input (conv_hpipe.hip): random (a, b) per (image, channel)
    float2* coef;
    RET(tmp.dalloc((void**)&coef, (size_t)B * Cin * sizeof(float2)));
    KCHK(launch_fill_random(DT_F32, coef, (size_t)B * Cin * 2, 3u, c->stream), "fill");
    o.gn_coef = coef; o.gn_relu = 1;
  }
  std::vector<OpFn> ops;
  RET(add_conv(&tmp, ops, L, xin, Cin, yout, Cout, image_segs(B, H, W, Ho, Wo), o));
  for (int i = 0; i < 2; ++i) RET(run_ops(c, ops, "bench_conv"));
  hipEvent_t e0, e1;
  HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
  HIPCHK(hipEventRecord(e0, c->stream));
  for (int i = 0; i < iters; ++i) RET(run_ops(c, ops, "bench_conv"));
  HIPCHK(hipEventRecord(e1, c->stream));
  HIPCHK(hipEventSynchronize(e1));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  if (ms_out) *ms_out = ms / (float)iters;
  if (flops_out) *flops_out = 2.0 * (double)B * Ho * Wo * Cout * K * K * Cin;
  return 0;
}

}  // extern "C"
