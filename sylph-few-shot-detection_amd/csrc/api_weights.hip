// Host side of libsylph_hip.so, unit "weights": checkpoint tensors -> packed device weights (sylph_load_weight / sylph_finalize_weights).
// No torch types, no CPU compute fallback: every stage is a HIP kernel from this directory.
#include "api_internal.h"

namespace sylph_host {

const HostTensor* find_w(sylph_ctx* c, const std::string& k) {
  auto it = c->host_w.find(k);
  return it == c->host_w.end() ? nullptr : &it->second;
}

// pack (Cout,Cin,KH,KW) fp32 -> [Cout_pad][KH][KW][Cin] compute dtype; several tensors may be stacked on Cout
int pack_conv(sylph_ctx* c, const std::vector<const HostTensor*>& ws, ConvLayer* L) {
  const HostTensor* w0 = ws[0];
  if (L->groups != 1) return fail("internal: pack_conv builds dense layers only (a grouped conv is packed by pack_conv_grouped)");
  if (w0->shape.size() != 4) return fail("conv weight must be 4-D");
  const int Cin = (int)w0->shape[1], KH = (int)w0->shape[2], KW = (int)w0->shape[3];
  int Cout = 0;
  for (auto* w : ws) {
    if ((int)w->shape[1] != Cin || (int)w->shape[2] != KH || (int)w->shape[3] != KW) return fail("stacked conv mismatch");
    Cout += (int)w->shape[0];
  }
  const int pad_to = Cout >= 128 ? 128 : (Cout > 32 ? 64 : 32);
  const int Cout_pad = (Cout + pad_to - 1) / pad_to * pad_to;
  const size_t K = (size_t)KH * KW * Cin;
  std::vector<float> packed((size_t)Cout_pad * K, 0.f);
  int n0 = 0;
  for (auto* w : ws) {
    const int co = (int)w->shape[0];
    for (int n = 0; n < co; ++n)
      for (int ci = 0; ci < Cin; ++ci)
        for (int kh = 0; kh < KH; ++kh)
          for (int kw = 0; kw < KW; ++kw)
            packed[(size_t)(n0 + n) * K + ((size_t)kh * KW + kw) * Cin + ci] =
                w->data[(((size_t)n * Cin + ci) * KH + kh) * KW + kw];
    n0 += co;
  }
  L->Cin = Cin; L->Cout = Cout; L->Cout_pad = Cout_pad; L->KH = KH; L->KW = KW;
  if (c->dt == DT_BF16) {
    std::vector<uint16_t> h(packed.size());
    for (size_t i = 0; i < packed.size(); ++i) h[i] = f2bf_host(packed[i]);
    RET(upload(c, &L->w, h.data(), h.size() * 2));
  } else if (c->dt == DT_F32S) {
    // split-bf16 parity mode (conv_igemm.hip MmaSplit): every 32-element K-slice of a row becomes [32 bf16 hi | 32 bf16 lo], the same
    // 128 bytes as its fp32 form; hi = bf16(w), lo = bf16(w - hi), both round-to-nearest-even
    if (K % 32 != 0) return fail("split-bf16 mode: K = KH * KW * Cin must be a multiple of 32");
    std::vector<uint16_t> h(packed.size() * 2);
    for (size_t i = 0; i < packed.size(); ++i) {
      const uint16_t hi = f2bf_host(packed[i]);
      uint32_t hb = (uint32_t)hi << 16;
      float hf;
      memcpy(&hf, &hb, 4);
      const size_t sl = i / 32, e = i % 32;
      h[sl * 64 + e] = hi;
      h[sl * 64 + 32 + e] = f2bf_host(packed[i] - hf);
    }
    RET(upload(c, &L->w, h.data(), h.size() * 2));
  } else {
    RET(upload(c, &L->w, packed.data(), packed.size() * 4));
  }
  return 0;
}

std::vector<uint16_t> pack_conv3x3_bf16(const float* w, int cout, int cout_pad) {
  std::vector<uint16_t> pk((size_t)cout_pad * 2304, 0);
  for (int n = 0; n < cout; ++n)
    for (int tap = 0; tap < 9; ++tap)
      for (int ci = 0; ci < 256; ++ci) pk[(size_t)n * 2304 + (size_t)tap * 256 + ci] = f2bf_host(w[w3x3_torch(n, tap, ci)]);
  return pk;
}

std::vector<uint16_t> pack_pred_taps(const float* w, int cout) {
  const int sw = (3 * cout + 3) & ~3;
  std::vector<uint16_t> tw((size_t)64 * 256, 0);
  for (int n = 0; n < cout; ++n)
    for (int tap = 0; tap < 9; ++tap)
      for (int ci = 0; ci < 256; ++ci) tw[(size_t)((tap / 3) * sw + (tap % 3) * cout + n) * 256 + ci] = f2bf_host(w[w3x3_torch(n, tap, ci)]);
  return tw;
}

int upload_vec(sylph_ctx* c, float** dev, const std::vector<float>& v, int pad_to) {
  std::vector<float> t(v);
  t.resize((size_t)pad_to, 0.f);
  return upload(c, (void**)dev, t.data(), t.size() * 4);
}

// conv + FrozenBN folded into per-channel scale/shift (detectron2 FrozenBatchNorm2d, eps 1e-5)
int make_conv_bn(sylph_ctx* c, const std::string& name, ConvLayer* L) {
  const HostTensor* w = find_w(c, name + ".weight");
  const HostTensor *g = find_w(c, name + ".norm.weight"), *b = find_w(c, name + ".norm.bias");
  const HostTensor *rm = find_w(c, name + ".norm.running_mean"), *rv = find_w(c, name + ".norm.running_var");
  if (!w || !g || !b || !rm || !rv) return fail("missing weights for " + name);
  RET(pack_conv(c, {w}, L));
  std::vector<float> sc(L->Cout), sh(L->Cout);
  for (int i = 0; i < L->Cout; ++i) {
    const float s = g->data[i] * (1.0f / sqrtf(rv->data[i] + 1e-5f));
    sc[i] = s;
    sh[i] = b->data[i] - rm->data[i] * s;
  }
  RET(upload_vec(c, &L->scale, sc, L->Cout_pad));
  RET(upload_vec(c, &L->shift, sh, L->Cout_pad));
  return 0;
}

// grouped 3x3 conv (ResNeXt conv2, detectron2 Conv2d(C, C, 3, groups=G)): weight (C, C / G, 3, 3) in conv_group.hip's layout,
// FrozenBN folded into scale / shift.  `key` names the weight in errors.
int pack_conv_grouped(sylph_ctx* c, const HostTensor& w, const std::string& key, int C, int groups, const float* scale, const float* shift,
                      ConvLayer* L) {
  if (groups < 1 || C % groups != 0) return fail(key + ": bad group count");
  const int cpg = C / groups;
  if (w.shape.size() != 4 || w.shape[0] != C || w.shape[1] != cpg || w.shape[2] != 3 || w.shape[3] != 3) {
    std::string got;
    for (size_t i = 0; i < w.shape.size(); ++i) got += (i ? ", " : "") + std::to_string(w.shape[i]);
    return fail(key + ": shape (" + got + ") where the config (MODEL.RESNETS.NUM_GROUPS " + std::to_string(groups) + ") needs (" +
                std::to_string(C) + ", " + std::to_string(cpg) + ", 3, 3)");
  }
  if (C % 64 != 0 || cpg < 4 || cpg > 64 || (cpg & (cpg - 1)) != 0)
    return fail(key + ": a grouped conv needs C % 64 == 0 and C / groups a power of two in [4, 64]");
  std::vector<uint8_t> packed(conv_group_packed_bytes(c->dt, C, cpg));
  conv_group_pack(c->dt, w.data.data(), C, cpg, packed.data());
  L->Cin = C; L->Cout = C; L->Cout_pad = C; L->KH = 3; L->KW = 3; L->groups = groups;
  RET(upload(c, &L->w, packed.data(), packed.size()));
  RET(upload_vec(c, &L->scale, std::vector<float>(scale, scale + C), C));
  RET(upload_vec(c, &L->shift, std::vector<float>(shift, shift + C), C));
  return 0;
}

// a bottleneck's conv2 + FrozenBN: (mid, mid / groups, 3, 3) checked against the config, grouped or dense
int make_conv2_bn(sylph_ctx* c, const std::string& name, int mid, int groups, ConvLayer* L) {
  const HostTensor* w = find_w(c, name + ".weight");
  if (w && (w->shape.size() != 4 || w->shape[0] != mid || w->shape[1] != mid / groups || w->shape[2] != 3 || w->shape[3] != 3)) {
    std::string got;
    for (size_t i = 0; i < w->shape.size(); ++i) got += (i ? ", " : "") + std::to_string(w->shape[i]);
    return fail(name + ".weight: shape (" + got + ") where the config (MODEL.RESNETS.NUM_GROUPS " + std::to_string(groups) +
                ", WIDTH_PER_GROUP " + std::to_string(c->cfg.width_per_group) + ") needs (" + std::to_string(mid) + ", " +
                std::to_string(mid / groups) + ", 3, 3)");
  }
  if (groups == 1) return make_conv_bn(c, name, L);
  const HostTensor *g = find_w(c, name + ".norm.weight"), *b = find_w(c, name + ".norm.bias");
  const HostTensor *rm = find_w(c, name + ".norm.running_mean"), *rv = find_w(c, name + ".norm.running_var");
  if (!w || !g || !b || !rm || !rv) return fail("missing weights for " + name);
  std::vector<float> sc(mid), sh(mid);
  for (int i = 0; i < mid; ++i) {
    const float s = g->data[i] * (1.0f / sqrtf(rv->data[i] + 1e-5f));
    sc[i] = s;
    sh[i] = b->data[i] - rm->data[i] * s;
  }
  return pack_conv_grouped(c, *w, name + ".weight", mid, groups, sc.data(), sh.data(), L);
}

// a backbone conv whose shape follows from MODEL.RESNETS.DEPTH (bottleneck or BasicBlock layout): a checkpoint of the other block type
// fails here, naming the key and the shape the config needs
static int expect_conv_shape(sylph_ctx* c, const std::string& name, int cout, int cin, int k) {
  const HostTensor* w = find_w(c, name + ".weight");
  const std::string need = "(" + std::to_string(cout) + ", " + std::to_string(cin) + ", " + std::to_string(k) + ", " + std::to_string(k) + ")";
  if (!w) return fail("missing weights for " + name + ".weight: MODEL.RESNETS.DEPTH " + std::to_string(c->cfg.resnet_depth) + " needs " + need);
  if (w->shape.size() != 4 || w->shape[0] != cout || w->shape[1] != cin || w->shape[2] != k || w->shape[3] != k) {
    std::string got;
    for (size_t i = 0; i < w->shape.size(); ++i) got += (i ? ", " : "") + std::to_string(w->shape[i]);
    return fail(name + ".weight: shape (" + got + ") where the config (MODEL.RESNETS.DEPTH " + std::to_string(c->cfg.resnet_depth) + ") needs " + need);
  }
  return 0;
}

int make_conv_bias(sylph_ctx* c, const std::vector<std::string>& names, ConvLayer* L) {
  std::vector<const HostTensor*> ws;
  std::vector<float> bias;
  for (auto& n : names) {
    const HostTensor *w = find_w(c, n + ".weight"), *b = find_w(c, n + ".bias");
    if (!w || !b) return fail("missing weights for " + n);
    ws.push_back(w);
    bias.insert(bias.end(), b->data.begin(), b->data.end());
  }
  RET(pack_conv(c, ws, L));
  RET(upload_vec(c, &L->shift, bias, L->Cout_pad));
  return 0;
}

// conv3 + projection shortcut as one pointwise layer over K = [conv3 inputs | shortcut inputs]: the two FrozenBN scales
// are folded into the weights in fp32 (before the dtype cast), the shifts are summed; no epilogue scale.
int make_c3sc(sylph_ctx* c, const HostTensor& w3, const float* s3, const float* h3, const HostTensor& ws, const float* ss,
                     const float* hs, ConvLayer* L) {
  const int co = (int)w3.shape[0], k3 = (int)w3.shape[1], ks = (int)ws.shape[1];
  HostTensor hc;
  hc.shape = {co, k3 + ks, 1, 1};
  hc.data.resize((size_t)co * (k3 + ks));
  std::vector<float> shift(co);
  for (int i = 0; i < co; ++i) {
    for (int k = 0; k < k3; ++k) hc.data[(size_t)i * (k3 + ks) + k] = w3.data[(size_t)i * k3 + k] * s3[i];
    for (int k = 0; k < ks; ++k) hc.data[(size_t)i * (k3 + ks) + k3 + k] = ws.data[(size_t)i * ks + k] * ss[i];
    shift[i] = h3[i] + hs[i];
  }
  RET(pack_conv(c, {&hc}, L));
  RET(upload_vec(c, &L->shift, shift, L->Cout_pad));
  return 0;
}

int make_gn(sylph_ctx* c, const std::string& name, GNLayer* G) {
  const HostTensor *g = find_w(c, name + ".weight"), *b = find_w(c, name + ".bias");
  if (!g || !b) return fail("missing weights for " + name);
  if (g->data.size() != 256) return fail("GroupNorm layers must have 256 channels: " + name);
  RET(upload_vec(c, &G->gamma, g->data, 256));
  RET(upload_vec(c, &G->beta, b->data, 256));
  return 0;
}

int upload_f32(sylph_ctx* c, const float** dev, const HostTensor* t, const std::string& what, size_t expect) {
  if (!t) return fail("missing weights for " + what);
  if (expect && t->data.size() != expect) return fail("unexpected size for " + what);
  void* d;
  RET(upload(c, &d, t->data.data(), t->data.size() * 4));
  *dev = (const float*)d;
  return 0;
}

int make_lin(sylph_ctx* c, const std::string& name, sylph_ctx::Lin* L) {
  const HostTensor *w = find_w(c, name + ".weight"), *b = find_w(c, name + ".bias");
  if (!w || !b || w->shape.size() != 2) return fail("missing weights for " + name);
  L->O = (int)w->shape[0]; L->K = (int)w->shape[1];
  RET(upload(c, (void**)&L->W, w->data.data(), w->data.size() * 4));
  RET(upload(c, (void**)&L->b, b->data.data(), b->data.size() * 4));
  return 0;
}

int make_ln(sylph_ctx* c, const std::string& name, GNLayer* G) {
  const HostTensor *g = find_w(c, name + ".weight"), *b = find_w(c, name + ".bias");
  if (!g || !b || g->data.size() != 256) return fail("missing weights for " + name);
  RET(upload_vec(c, &G->gamma, g->data, 256));
  RET(upload_vec(c, &G->beta, b->data, 256));
  return 0;
}

// ---- MobileNetV2 (cfg.mobilenet) ----------------------------------------------------------------------------------------------------
static std::string shape_str(const HostTensor& t) {
  std::string got;
  for (size_t i = 0; i < t.shape.size(); ++i) got += (i ? ", " : "") + std::to_string(t.shape[i]);
  return "(" + got + ")";
}

// a dense 1x1 conv (cout, cin, 1, 1) stored as (cout_p, cin_p): zero rows / columns, zero scale and shift on the pad channels
static int make_padded_1x1(sylph_ctx* c, const HostTensor& w, int cout, int cin, int cout_p, int cin_p, const float* scale, const float* shift, ConvLayer* L) {
  HostTensor hp;
  hp.shape = {cout_p, cin_p, 1, 1};
  hp.data.assign((size_t)cout_p * cin_p, 0.f);
  for (int n = 0; n < cout; ++n)
    for (int k = 0; k < cin; ++k) hp.data[(size_t)n * cin_p + k] = w.data[(size_t)n * cin + k];
  RET(pack_conv(c, {&hp}, L));
  if (scale) RET(upload_vec(c, &L->scale, std::vector<float>(scale, scale + cout), L->Cout_pad));  // (nullptr: a bias conv, as make_conv_bias packs it)
  RET(upload_vec(c, &L->shift, std::vector<float>(shift, shift + cout), L->Cout_pad));
  return 0;
}

// depthwise weights (C, 1, 3, 3) -> fp32 [3][3][Cp] (bf16 mode: the values a bf16 weight holds), scale / shift [Cp], zeros on the pad channels
int make_dw_table(sylph_ctx* c, const HostTensor& w, int C, int Cp, const float* scale, const float* shift, float** w_dev, float** scale_dev, float** shift_dev) {
  std::vector<float> t((size_t)9 * Cp, 0.f);
  for (int ch = 0; ch < C; ++ch)
    for (int tap = 0; tap < 9; ++tap) {
      float v = w.data[(size_t)ch * 9 + tap];
      if (c->dt == DT_BF16) {
        const uint32_t u = (uint32_t)f2bf_host(v) << 16;
        memcpy(&v, &u, 4);
      }
      t[(size_t)tap * Cp + ch] = v;
    }
  RET(upload(c, (void**)w_dev, t.data(), t.size() * 4));
  RET(upload_vec(c, scale_dev, std::vector<float>(scale, scale + C), Cp));
  RET(upload_vec(c, shift_dev, std::vector<float>(shift, shift + C), Cp));
  return 0;
}

int make_mbv2_block(sylph_ctx* c, int cin, int t, int cout, int stride, const HostTensor* const* w, const float* const* scale, const float* const* shift,
                    sylph_ctx::MbBlock* blk) {
  const int hid = cin * t;
  blk->cin = cin; blk->t = t; blk->cout = cout; blk->stride = stride;
  blk->cin_p = mbv2_pad(c, cin); blk->hid_p = mbv2_pad(c, hid); blk->cout_p = mbv2_pad(c, cout);
  blk->cin_ld = mbv2_ld(c, cin); blk->hid_ld = mbv2_ld(c, hid); blk->cout_ld = mbv2_ld(c, cout);
  if (t != 1) RET(make_padded_1x1(c, *w[0], hid, cin, blk->hid_p, blk->cin_p, scale[0], shift[0], &blk->exp));
  RET(make_dw_table(c, *w[1], hid, blk->hid_p, scale[1], shift[1], &blk->dw_w, &blk->dw_scale, &blk->dw_shift));
  RET(make_padded_1x1(c, *w[2], cout, hid, blk->cout_p, blk->hid_p, scale[2], shift[2], &blk->proj));
  if ((t != 1 && blk->exp.Cout_pad != blk->hid_ld) || blk->proj.Cout_pad != blk->cout_ld) return fail("internal: MobileNetV2 row pitch");
  if (c->dt == DT_BF16) {  // the same two matrices row-major in bf16, zero on the pad channels, for the one-launch block (conv_mbv2.hip)
    auto pack = [&](const HostTensor& src, int rows, int cols, int rows_p, int cols_p, bf16_t** dev) {
      std::vector<uint16_t> m((size_t)rows_p * cols_p, 0);
      for (int n = 0; n < rows; ++n)
        for (int k = 0; k < cols; ++k) m[(size_t)n * cols_p + k] = f2bf_host(src.data[(size_t)n * cols + k]);
      return upload(c, (void**)dev, m.data(), m.size() * 2);
    };
    if (t != 1) RET(pack(*w[0], hid, cin, blk->hid_p, blk->cin_p, &blk->fw1));
    RET(pack(*w[2], cout, hid, blk->cout_p, blk->hid_p, &blk->fw2));
  }
  return 0;
}

// conv `wkey`.weight of shape (cout, cin_w, k, k) + torch-style FrozenBN `bnkey`.{weight, bias, running_mean, running_var} (eps 1e-5)
static int mbv2_conv_bn(sylph_ctx* c, const std::string& wkey, const std::string& bnkey, int cout, int cin_w, int k, const HostTensor** w,
                        std::vector<float>* sc, std::vector<float>* sh) {
  const std::string need = "(" + std::to_string(cout) + ", " + std::to_string(cin_w) + ", " + std::to_string(k) + ", " + std::to_string(k) + ")";
  *w = find_w(c, wkey + ".weight");
  if (!*w) return fail("missing weights for " + wkey + ".weight: MODEL.MOBILENET needs " + need);
  if ((*w)->shape != std::vector<int64_t>{cout, cin_w, k, k}) return fail(wkey + ".weight: shape " + shape_str(**w) + " where MODEL.MOBILENET needs " + need);
  const HostTensor *g = find_w(c, bnkey + ".weight"), *b = find_w(c, bnkey + ".bias");
  const HostTensor *rm = find_w(c, bnkey + ".running_mean"), *rv = find_w(c, bnkey + ".running_var");
  if (!g || !b || !rm || !rv) return fail("missing weights for " + bnkey);
  if ((int)g->data.size() != cout || (int)b->data.size() != cout || (int)rm->data.size() != cout || (int)rv->data.size() != cout)
    return fail(bnkey + ": FrozenBN tensors must have " + std::to_string(cout) + " elements");
  sc->resize(cout); sh->resize(cout);
  for (int i = 0; i < cout; ++i) {
    const float s = g->data[i] * (1.0f / sqrtf(rv->data[i] + 1e-5f));
    (*sc)[i] = s;
    (*sh)[i] = b->data[i] - rm->data[i] * s;
  }
  return 0;
}

// AdelaiDet MobileNetV2 (tonylins layout, width 1.0): features.0 = conv 3x3 s2 + BN + ReLU6, features.1..17 = InvertedResidual blocks of
// the (t, c, n, s) table; FPN laterals on res3 / res4 / res5 = features 6 / 13 / 17 (32 / 96 / 320 channels)
static int finalize_mbv2(sylph_ctx* c) {
  const std::string f = "backbone.bottom_up.features.";
  {
    const HostTensor* w;
    std::vector<float> sc, sh;
    RET(mbv2_conv_bn(c, f + "0.0", f + "0.1", 32, 3, 3, &w, &sc, &sh));
    std::vector<float> t((size_t)9 * 4 * 32, 0.f);
    for (int n = 0; n < 32; ++n)
      for (int ch = 0; ch < 3; ++ch)
        for (int tap = 0; tap < 9; ++tap) {
          float v = w->data[((size_t)n * 3 + ch) * 9 + tap];
          if (c->dt == DT_BF16) {
            const uint32_t u = (uint32_t)f2bf_host(v) << 16;
            memcpy(&v, &u, 4);
          }
          t[((size_t)tap * 4 + ch) * 32 + n] = v;
        }
    RET(upload(c, (void**)&c->mb_stem_w, t.data(), t.size() * 4));
    RET(upload_vec(c, &c->mb_stem_scale, sc, 32));
    RET(upload_vec(c, &c->mb_stem_shift, sh, 32));
  }
  const int table[7][4] = {{1, 16, 1, 1}, {6, 24, 2, 2}, {6, 32, 3, 2}, {6, 64, 4, 2}, {6, 96, 3, 1}, {6, 160, 3, 2}, {6, 320, 1, 1}};
  int cin = 32, fi = 1;
  c->mb_blocks.clear();
  for (auto& row : table)
    for (int i = 0; i < row[2]; ++i, ++fi) {
      const int t = row[0], cout = row[1], stride = i == 0 ? row[3] : 1, hid = cin * t;
      const std::string q = f + std::to_string(fi) + ".conv.";
      const HostTensor* w[3] = {nullptr, nullptr, nullptr};
      std::vector<float> sc[3], sh[3];
      const int j = t == 1 ? 0 : 3;  // nn.Sequential index of the depthwise conv
      if (t != 1) RET(mbv2_conv_bn(c, q + "0", q + "1", hid, cin, 1, &w[0], &sc[0], &sh[0]));
      RET(mbv2_conv_bn(c, q + std::to_string(j), q + std::to_string(j + 1), hid, 1, 3, &w[1], &sc[1], &sh[1]));
      RET(mbv2_conv_bn(c, q + std::to_string(j + 3), q + std::to_string(j + 4), cout, hid, 1, &w[2], &sc[2], &sh[2]));
      const float* scp[3] = {sc[0].data(), sc[1].data(), sc[2].data()};
      const float* shp[3] = {sh[0].data(), sh[1].data(), sh[2].data()};
      c->mb_blocks.emplace_back();
      RET(make_mbv2_block(c, cin, t, cout, stride, w, scp, shp, &c->mb_blocks.back()));
      cin = cout;
    }
  const int lat_c[3] = {32, 96, 320};
  for (int k = 0; k < 3; ++k) {
    const std::string name = "backbone.fpn_lateral" + std::to_string(k + 3);
    const HostTensor *lw = find_w(c, name + ".weight"), *lb = find_w(c, name + ".bias");
    if (!lw || !lb) return fail("missing weights for " + name);
    if (lw->shape != std::vector<int64_t>{256, lat_c[k], 1, 1} || lb->data.size() != 256)
      return fail(name + ".weight: shape " + shape_str(*lw) + " where MODEL.MOBILENET needs (256, " + std::to_string(lat_c[k]) + ", 1, 1)");
    RET(make_padded_1x1(c, *lw, 256, lat_c[k], 256, mbv2_pad(c, lat_c[k]), nullptr, lb->data.data(), &c->fpn_lat[k]));
    RET(make_conv_bias(c, {"backbone.fpn_output" + std::to_string(k + 3)}, &c->fpn_out[k]));
  }
  RET(make_conv_bias(c, {"backbone.top_block.p6"}, &c->p6));
  RET(make_conv_bias(c, {"backbone.top_block.p7"}, &c->p7));
  c->has_backbone = true;
  return 0;
}

bool has_prefix(sylph_ctx* c, const std::string& p) {
  auto it = c->host_w.lower_bound(p);
  return it != c->host_w.end() && it->first.compare(0, p.size(), p) == 0;
}

}  // namespace sylph_host

extern "C" {

int sylph_load_weight(sylph_ctx* c, const char* name, const float* data, const int64_t* shape, int ndim) {
  if (c->finalized) return fail("weights already finalized");
  HostTensor t;
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
  t.data.assign(data, data + n);
  c->host_w[name] = std::move(t);
  return 0;
}

int sylph_finalize_weights(sylph_ctx* c) {
  if (c->finalized) return fail("weights already finalized");
  HIPCHK(hipSetDevice(c->device));
  const std::string bu = "backbone.bottom_up";
  if (c->cfg.mobilenet) {
    if (has_prefix(c, bu + ".stem") || has_prefix(c, bu + ".res"))
      return fail("MODEL.MOBILENET: the checkpoint holds ResNet keys (" + bu + ".stem / .res*) where " + bu + ".features.* are needed");
    if (has_prefix(c, bu + ".features.")) RET(finalize_mbv2(c));
  } else if (has_prefix(c, bu + ".features.")) {
    return fail("the checkpoint holds MobileNetV2 keys (" + bu + ".features.*): set MODEL.MOBILENET True");
  } else if (has_prefix(c, bu + ".stem")) {
    const HostTensor* w = find_w(c, bu + ".stem.conv1.weight");
    const HostTensor *g = find_w(c, bu + ".stem.conv1.norm.weight"), *b = find_w(c, bu + ".stem.conv1.norm.bias");
    const HostTensor *rm = find_w(c, bu + ".stem.conv1.norm.running_mean"),
                     *rv = find_w(c, bu + ".stem.conv1.norm.running_var");
    if (!w || !g || !b || !rm || !rv) return fail("missing stem weights");
    if (w->shape[0] != 64 || w->shape[1] != 3 || w->shape[2] != 7 || w->shape[3] != 7) return fail("stem must be 64x3x7x7");
    {
      // Stem as an implicit GEMM (conv_igemm.hip, stem loader): K-slice s = RPS kernel rows of an
      // 8-pixel x 4-channel window; window pixel 0, channel 3 and kernel rows >= 7 carry zeros.
      const int BK = c->dt == DT_BF16 ? 64 : 32, RPS = BK / 32, NS = (7 + RPS - 1) / RPS;
      HostTensor hs;
      hs.shape = {64, BK, NS, 1};
      hs.data.assign((size_t)64 * BK * NS, 0.f);
      for (int n = 0; n < 64; ++n)
        for (int s = 0; s < NS; ++s)
          for (int e = 0; e < BK; ++e) {
            const int kh = s * RPS + e / 32, px = (e % 32) / 4, ch = e % 4, kw = px - 1;
            if (kh < 7 && kw >= 0 && kw < 7 && ch < 3)
              hs.data[((size_t)n * BK + e) * NS + s] = w->data[((n * 3 + ch) * 7 + kh) * 7 + kw];
          }
      RET(pack_conv(c, {&hs}, &c->stem));
      std::vector<float> sc(64), sh(64);
      for (int i = 0; i < 64; ++i) {
        sc[i] = g->data[i] * (1.0f / sqrtf(rv->data[i] + 1e-5f));
        sh[i] = b->data[i] - rm->data[i] * sc[i];
      }
      RET(upload_vec(c, &c->stem.scale, sc, c->stem.Cout_pad));
      RET(upload_vec(c, &c->stem.shift, sh, c->stem.Cout_pad));
      if (c->dt == DT_BF16) {  // dedicated stem kernel: [n][kh][8 px][4 ch], kernel column 7 / channel 3 zero
        std::vector<bf16_t> wp((size_t)64 * 224);
        for (int n = 0; n < 64; ++n)
          for (int kh = 0; kh < 7; ++kh)
            for (int px = 0; px < 8; ++px)
              for (int ch = 0; ch < 4; ++ch)
                wp[(size_t)n * 224 + kh * 32 + px * 4 + ch] =
                    (bf16_t)((px < 7 && ch < 3) ? w->data[((n * 3 + ch) * 7 + kh) * 7 + px] : 0.f);
        RET(upload(c, &c->stem_wp, wp.data(), wp.size() * sizeof(bf16_t)));
      }
    }
    const int nb50[4] = {3, 4, 6, 3}, nb101[4] = {3, 4, 23, 3}, nb152[4] = {3, 8, 36, 3};
    const int nb18[4] = {2, 2, 2, 2}, nb34[4] = {3, 4, 6, 3};
    const bool basic = c->cfg.resnet_depth == 18 || c->cfg.resnet_depth == 34;
    const int* nb = c->cfg.resnet_depth == 18 ? nb18 : c->cfg.resnet_depth == 34 ? nb34 :
                    c->cfg.resnet_depth == 50 ? nb50 : (c->cfg.resnet_depth == 101 ? nb101 : nb152);
    c->stages.resize(4);
    for (int si = 0; si < 4; ++si) {
      c->stages[si].resize(nb[si]);
      for (int bi = 0; bi < nb[si]; ++bi) {
        const std::string q = bu + ".res" + std::to_string(si + 2) + "." + std::to_string(bi);
        auto& blk = c->stages[si][bi];
        if (basic) {
          // detectron2 BasicBlock: conv1 3x3 (stride) -> conv2 3x3, stage width 64 << si, a projection shortcut only where the width changes
          const int cout = 64 << si, cin = (bi == 0 && si > 0) ? cout / 2 : cout;
          blk.basic = true;
          RET(expect_conv_shape(c, q + ".conv1", cout, cin, 3));
          RET(make_conv_bn(c, q + ".conv1", &blk.c1));
          RET(expect_conv_shape(c, q + ".conv2", cout, cout, 3));
          RET(make_conv_bn(c, q + ".conv2", &blk.c2));
          blk.has_sc = cin != cout;
          if (blk.has_sc) {
            RET(expect_conv_shape(c, q + ".shortcut", cout, cin, 1));
            RET(make_conv_bn(c, q + ".shortcut", &blk.sc));
          }
          continue;
        }
        if (const HostTensor* w1 = find_w(c, q + ".conv1.weight"))  // a BasicBlock checkpoint (3x3 conv1) under a bottleneck depth
          if (w1->shape.size() == 4 && (w1->shape[2] != 1 || w1->shape[3] != 1))
            return expect_conv_shape(c, q + ".conv1", (c->cfg.num_groups * c->cfg.width_per_group) << si,
                                     bi > 0 ? 256 << si : (si == 0 ? 64 : 128 << si), 1);
        RET(make_conv_bn(c, q + ".conv1", &blk.c1));
        RET(make_conv2_bn(c, q + ".conv2", (c->cfg.num_groups * c->cfg.width_per_group) << si, c->cfg.num_groups, &blk.c2));
        RET(make_conv_bn(c, q + ".conv3", &blk.c3));
        blk.has_sc = bi == 0;
        if (blk.has_sc) RET(make_conv_bn(c, q + ".shortcut", &blk.sc));
        if (blk.has_sc && knob::fuse_shortcut()) {
          // fold the two FrozenBN scales into the weights, sum the shifts (fp32 before the dtype cast)
          const HostTensor *w3 = find_w(c, q + ".conv3.weight"), *ws = find_w(c, q + ".shortcut.weight");
          const int co = (int)w3->shape[0];
          std::vector<float> s3(co), h3(co), ss(co), hs(co);
          for (int i = 0; i < co; ++i) {
            const float a3 = find_w(c, q + ".conv3.norm.weight")->data[i] *
                             (1.0f / sqrtf(find_w(c, q + ".conv3.norm.running_var")->data[i] + 1e-5f));
            s3[i] = a3;
            h3[i] = find_w(c, q + ".conv3.norm.bias")->data[i] - find_w(c, q + ".conv3.norm.running_mean")->data[i] * a3;
            const float as = find_w(c, q + ".shortcut.norm.weight")->data[i] *
                             (1.0f / sqrtf(find_w(c, q + ".shortcut.norm.running_var")->data[i] + 1e-5f));
            ss[i] = as;
            hs[i] = find_w(c, q + ".shortcut.norm.bias")->data[i] - find_w(c, q + ".shortcut.norm.running_mean")->data[i] * as;
          }
          RET(make_c3sc(c, *w3, s3.data(), h3.data(), *ws, ss.data(), hs.data(), &blk.c3sc));
          blk.fused_sc = true;
        }
      }
    }
    for (int k = 0; k < 3; ++k) {
      if (basic) {
        const HostTensor* lw = find_w(c, "backbone.fpn_lateral" + std::to_string(k + 3) + ".weight");
        if (lw && (lw->shape.size() != 4 || lw->shape[1] != (128 << k)))
          return fail("backbone.fpn_lateral" + std::to_string(k + 3) + ".weight: MODEL.RESNETS.DEPTH " + std::to_string(c->cfg.resnet_depth) +
                      " needs (256, " + std::to_string(128 << k) + ", 1, 1)");
      }
      RET(make_conv_bias(c, {"backbone.fpn_lateral" + std::to_string(k + 3)}, &c->fpn_lat[k]));
      RET(make_conv_bias(c, {"backbone.fpn_output" + std::to_string(k + 3)}, &c->fpn_out[k]));
    }
    RET(make_conv_bias(c, {"backbone.top_block.p6"}, &c->p6));
    RET(make_conv_bias(c, {"backbone.top_block.p7"}, &c->p7));
    c->has_backbone = true;
  }
  const std::string hp = "proposal_generator.fcos_head";
  if (has_prefix(c, hp + ".cls_tower") || has_prefix(c, hp + ".bbox_tower")) {
    c->cls_tower.resize(c->cfg.num_cls_convs); c->cls_gn.resize(c->cfg.num_cls_convs);
    c->box_tower.resize(c->cfg.num_box_convs); c->box_gn.resize(c->cfg.num_box_convs);
    c->share_tower.resize(c->cfg.num_share_convs); c->share_gn.resize(c->cfg.num_share_convs);
    // nn.Sequential indices of a tower (fcos.py:72-122): conv 3 i, norm 3 i + 1, ReLU 3 i + 2 -- without a norm layer conv 2 i, ReLU 2 i + 1
    const bool gn = c->cfg.tower_norm == 0;
    const int step = gn ? 3 : 2;
    struct { const char* name; std::vector<ConvLayer>* convs; std::vector<GNLayer>* gns; int n; } towers[3] = {
        {".cls_tower.", &c->cls_tower, &c->cls_gn, c->cfg.num_cls_convs}, {".bbox_tower.", &c->box_tower, &c->box_gn, c->cfg.num_box_convs},
        {".share_tower.", &c->share_tower, &c->share_gn, c->cfg.num_share_convs}};
    ConvLayer* offs[3] = {&c->cls_off, &c->box_off, nullptr};
    c->cls_off = ConvLayer(); c->box_off = ConvLayer();
    for (int ti = 0; ti < 3; ++ti) {
      auto& t = towers[ti];
      for (int i = 0; i < t.n; ++i) {
        const std::string k = hp + t.name + std::to_string(step * i);
        if (c->cfg.tower_deformable && offs[ti] && i + 1 == t.n) {
          // MODEL.FCOS.USE_DEFORMABLE (fcos.py:83-84): the last conv is adet's DFConv2d -- offset conv (27 = 2 x 9 offsets + 9 mask
          // logits) and the modulated deformable conv itself (conv_deform.hip)
          for (const char* sfx : {".offset.weight", ".offset.bias", ".conv.weight", ".conv.bias"})
            if (!find_w(c, k + sfx)) return fail("MODEL.FCOS.USE_DEFORMABLE: missing checkpoint key " + k + sfx);
          const HostTensor *ow = find_w(c, k + ".offset.weight"), *cw = find_w(c, k + ".conv.weight");
          if (ow->shape != std::vector<int64_t>{27, 256, 3, 3}) return fail(k + ".offset.weight must be [27, 256, 3, 3] (modulated, one deformable group)");
          if (cw->shape != std::vector<int64_t>{256, 256, 3, 3}) return fail(k + ".conv.weight must be [256, 256, 3, 3]");
          if (find_w(c, k + ".offset.bias")->data.size() != 27 || find_w(c, k + ".conv.bias")->data.size() != 256)
            return fail(k + ".offset.bias / .conv.bias must have 27 / 256 elements");
          RET(make_conv_bias(c, {k + ".offset"}, offs[ti]));
          // split-bf16 parity mode: conv_deform.hip runs this layer with exact fp32 MFMAs on fp32-packed weights
          const DType keep = c->dt;
          if (keep == DT_F32S) c->dt = DT_F32;
          const int rc = make_conv_bias(c, {k + ".conv"}, &(*t.convs)[i]);
          c->dt = keep;
          RET(rc);
        } else {
          RET(make_conv_bias(c, {k}, &(*t.convs)[i]));
        }
        if (gn) RET(make_gn(c, hp + t.name + std::to_string(step * i + 1), &(*t.gns)[i]));
      }
    }
    RET(make_conv_bias(c, {hp + ".bbox_pred", hp + ".ctrness", hp + ".iou_overlap"}, &c->pred));
    if (find_w(c, hp + ".cls_logits.weight") && find_w(c, hp + ".cls_logits.bias")) {
      const HostTensor* w = find_w(c, hp + ".cls_logits.weight");
      if (w->shape.size() == 4 && w->shape[1] == 256 && w->shape[2] == w->shape[3] && (w->shape[2] == 1 || w->shape[2] == 3)) {
        RET(make_conv_bias(c, {hp + ".cls_logits"}, &c->cls_logits));
        c->has_cls_logits = true;
      }
    }
    // the box branch as finalized, stacked in torch order: what sylph_get_box_branch returns and a reset of sylph_set_box_branch restores
    c->box_w0.clear(); c->box_b0.clear();
    if (c->pred.KH == 3 && c->pred.KW == 3 && c->pred.Cin == 256)
      for (const char* nm : {".bbox_pred", ".ctrness", ".iou_overlap"}) {
        const HostTensor *w = find_w(c, hp + nm + ".weight"), *b = find_w(c, hp + nm + ".bias");
        c->box_w0.insert(c->box_w0.end(), w->data.begin(), w->data.end());
        c->box_b0.insert(c->box_b0.end(), b->data.begin(), b->data.end());
      }
    c->pred_taps = nullptr;
    if (c->dt == DT_BF16 && !c->box_w0.empty() && 3 * ((3 * c->pred.Cout + 3) & ~3) <= 64) {
      // the same weights as the tap table of the fused GroupNorm + prediction pass
      const std::vector<uint16_t> tw = pack_pred_taps(c->box_w0.data(), c->pred.Cout);
      RET(upload(c, &c->pred_taps, tw.data(), tw.size() * 2));
    }
    c->level_scales.assign(c->cfg.nlevels, 1.f);
    if (c->cfg.use_scale)
      for (int l = 0; l < c->cfg.nlevels; ++l) {
        const HostTensor* s = find_w(c, hp + ".scales." + std::to_string(l) + ".scale");
        if (!s) return fail("missing " + hp + ".scales." + std::to_string(l) + ".scale");
        c->level_scales[l] = s->data[0];
      }
    c->box_s0 = c->level_scales;
    c->box_w = c->box_w0; c->box_b = c->box_b0;
    c->box_stamp = 0;
    c->has_head = true;
  }
  const std::string cp = "code_generator.code_generator_head";
  if (has_prefix(c, cp)) {
    c->cg_tower.resize(c->cfg.cg_tower_layers); c->cg_gn.resize(c->cfg.cg_tower_layers);
    int seq = 0;  // nn.Sequential index: conv, then the norm / activation modules that exist (code_generator.py:648-688)
    for (int i = 0; i < c->cfg.cg_tower_layers; ++i) {
      RET(make_conv_bias(c, {cp + ".support_set_shared_tower." + std::to_string(seq)}, &c->cg_tower[i]));
      ++seq;
      if ((c->cfg.cg_tower_gn_mask >> i) & 1) {
        RET(make_gn(c, cp + ".support_set_shared_tower." + std::to_string(seq), &c->cg_gn[i]));
        ++seq;
      }
      if ((c->cfg.cg_tower_relu_mask >> i) & 1) ++seq;
    }
    RET(make_conv_bias(c, {cp + ".support_set_cls_conv.0"}, &c->cg_cls));
    {
      std::vector<std::string> aux;
      if (c->cfg.cg_has_bias) { c->cg_ib = (int)aux.size(); aux.push_back(cp + ".support_set_cls_bias.0"); }
      if (c->cfg.cg_has_weight) { c->cg_iw = (int)aux.size(); aux.push_back(cp + ".support_set_cls_weight.0"); }
      if (c->cfg.cg_has_scale) { c->cg_is = (int)aux.size(); aux.push_back(cp + ".support_set_cls_scale.0"); }
      c->cg_naux = (int)aux.size();
      if (!aux.empty()) RET(make_conv_bias(c, aux, &c->cg_bias));
    }
    if (c->cfg.cg_post_norm) RET(make_gn(c, cp + ".post_norm", &c->cg_post));
    // conv_scale exists iff USE_WEIGHT_SCALE and (CONV_L2_NORM or POST_NORM)  (code_generator.py:372-374)
    c->cg_conv_scale = 1.f;
    if (c->cfg.cg_use_weight_scale && (c->cfg.cg_conv_l2_norm || c->cfg.cg_post_norm)) {
      const HostTensor* s = find_w(c, cp + ".conv_scale.scale");
      if (!s) return fail("missing " + cp + ".conv_scale.scale");
      c->cg_conv_scale = s->data[0];
    }
    c->cg_bias_scale = 1.f;
    if (c->cfg.cg_has_bias) {
      const HostTensor* s = find_w(c, cp + ".bias_scale.scale");
      if (!s) return fail("missing " + cp + ".bias_scale.scale");
      c->cg_bias_scale = s->data[0];
    }
    c->cg_bias_prior = -logf((1.f - c->cfg.prior_prob) / c->cfg.prior_prob);
    if (c->cfg.cg_meta_bias) {
      const HostTensor* bv = find_w(c, cp + ".bias_value");
      if (!bv || bv->data.empty()) return fail("META_BIAS is set but " + cp + ".bias_value is missing from the checkpoint");
      c->cg_bias_prior = bv->data[0];
    }
    c->has_codegen = true;
    capture_code_generator(c);
  }
  if (c->cfg.cg_type == 1 && has_prefix(c, "code_generator.box_pooler")) {
    const std::string rp = "code_generator";
    auto& R = c->re;
    RET(make_conv_bias(c, {rp + ".box_pooler.conv.0"}, &R.pool_conv));
    RET(make_gn(c, rp + ".box_pooler.conv.1", &R.pool_gn));
    const std::string cam = rp + ".box_pooler.context_attention_module";
    RET(upload_f32(c, &R.cam.l_w1, find_w(c, cam + ".local_att.0.weight"), cam, 64 * 256));
    RET(upload_f32(c, &R.cam.l_b1, find_w(c, cam + ".local_att.0.bias"), cam, 64));
    RET(upload_f32(c, &R.cam.l_g1, find_w(c, cam + ".local_att.1.weight"), cam, 64));
    RET(upload_f32(c, &R.cam.l_be1, find_w(c, cam + ".local_att.1.bias"), cam, 64));
    RET(upload_f32(c, &R.cam.l_w2, find_w(c, cam + ".local_att.3.weight"), cam, 256 * 64));
    RET(upload_f32(c, &R.cam.l_b2, find_w(c, cam + ".local_att.3.bias"), cam, 256));
    RET(upload_f32(c, &R.cam.l_g2, find_w(c, cam + ".local_att.4.weight"), cam, 256));
    RET(upload_f32(c, &R.cam.l_be2, find_w(c, cam + ".local_att.4.bias"), cam, 256));
    RET(upload_f32(c, &R.cam.g_w1, find_w(c, cam + ".global_att.1.weight"), cam, 64 * 256));
    RET(upload_f32(c, &R.cam.g_b1, find_w(c, cam + ".global_att.1.bias"), cam, 64));
    RET(upload_f32(c, &R.cam.g_g1, find_w(c, cam + ".global_att.2.weight"), cam, 64));
    RET(upload_f32(c, &R.cam.g_be1, find_w(c, cam + ".global_att.2.bias"), cam, 64));
    RET(upload_f32(c, &R.cam.g_w2, find_w(c, cam + ".global_att.4.weight"), cam, 256 * 64));
    RET(upload_f32(c, &R.cam.g_b2, find_w(c, cam + ".global_att.4.bias"), cam, 256));
    RET(upload_f32(c, &R.cam.g_g2, find_w(c, cam + ".global_att.5.weight"), cam, 256));
    RET(upload_f32(c, &R.cam.g_be2, find_w(c, cam + ".global_att.5.bias"), cam, 256));
    R.tok_conv.resize(c->cfg.tok_num_conv); R.tok_gn.resize(c->cfg.tok_num_conv);
    for (int k = 0; k < c->cfg.tok_num_conv; ++k) {
      const std::string q = rp + ".tokenizer.conv" + std::to_string(k + 1);
      const HostTensor* w = find_w(c, q + ".weight");
      if (!w) return fail("missing weights for " + q);
      if (find_w(c, q + ".bias")) return fail(q + ": a conv bias together with TOKENIZER.NORM is not supported");
      RET(pack_conv(c, {w}, &R.tok_conv[k]));
      RET(make_gn(c, q + ".norm", &R.tok_gn[k]));
    }
    if (c->cfg.tok_num_fc < 1) return fail("TOKENIZER.NUM_FC must be >= 1");
    R.tok_fc.resize(c->cfg.tok_num_fc);
    for (int k = 0; k < c->cfg.tok_num_fc; ++k) {
      const std::string q = rp + ".tokenizer.fc" + std::to_string(k + 1);
      if (k == 0) {
        // nn.Flatten order is (c, p); activations here are position-major (p, c): permute the columns once
        HostTensor* w = const_cast<HostTensor*>(find_w(c, q + ".weight"));
        if (!w || w->shape.size() != 2 || w->shape[1] != 256 * 49) return fail("tokenizer.fc1 must take 256*7*7 inputs");
        std::vector<float> perm(w->data.size());
        const int O = (int)w->shape[0];
        for (int o = 0; o < O; ++o)
          for (int ch = 0; ch < 256; ++ch)
            for (int pp = 0; pp < 49; ++pp) perm[(size_t)o * 12544 + pp * 256 + ch] = w->data[(size_t)o * 12544 + ch * 49 + pp];
        w->data.swap(perm);
      }
      RET(make_lin(c, q, &R.tok_fc[k]));
      if (R.tok_fc[k].O != 256) return fail("TOKENIZER.FC_DIM must be 256");
    }
    R.layers.resize(c->cfg.enc_layers);
    for (int l = 0; l < c->cfg.enc_layers; ++l) {
      const std::string q = rp + ".transformer_encoder.layers." + std::to_string(l);
      const HostTensor *ipw = find_w(c, q + ".self_attn.in_proj_weight"), *ipb = find_w(c, q + ".self_attn.in_proj_bias");
      const HostTensor *ow = find_w(c, q + ".self_attn.out_proj.weight"), *ob = find_w(c, q + ".self_attn.out_proj.bias");
      if (!ipw || !ipb || !ow || !ob || ipw->data.size() != 3 * 256 * 256) return fail("missing weights for " + q);
      // sequence length 1 => attention weights are 1: SA(x) = Wo (Wv x + bv) + bo, folded into one matrix
      HostTensor fw, fb;
      fw.shape = {256, 256}; fw.data.resize(256 * 256);
      fb.shape = {256}; fb.data.resize(256);
      const float* Wv = ipw->data.data() + 2 * 256 * 256;
      const float* bv = ipb->data.data() + 2 * 256;
      for (int i = 0; i < 256; ++i) {
        for (int k = 0; k < 256; ++k) {
          double a = 0.0;
          for (int j = 0; j < 256; ++j) a += (double)ow->data[i * 256 + j] * (double)Wv[j * 256 + k];
          fw.data[i * 256 + k] = (float)a;
        }
        double bb = ob->data[i];
        for (int j = 0; j < 256; ++j) bb += (double)ow->data[i * 256 + j] * (double)bv[j];
        fb.data[i] = (float)bb;
      }
      c->host_w[q + ".folded_attn.weight"] = fw;
      c->host_w[q + ".folded_attn.bias"] = fb;
      RET(make_lin(c, q + ".folded_attn", &R.layers[l].attn));
      RET(make_lin(c, q + ".linear1", &R.layers[l].l1));
      RET(make_lin(c, q + ".linear2", &R.layers[l].l2));
      RET(make_ln(c, q + ".norm1", &R.layers[l].n1));
      RET(make_ln(c, q + ".norm2", &R.layers[l].n2));
    }
    if (c->cfg.head_num_fc < 1 || c->cfg.head_num_fc > 2) return fail("HEAD.NUM_FC must be 1 or 2");
    R.wh.resize(c->cfg.head_num_fc); R.bh.resize(c->cfg.head_num_fc);
    for (int k = 0; k < c->cfg.head_num_fc; ++k) {
      RET(make_lin(c, rp + ".weight_head.fc" + std::to_string(k + 1), &R.wh[k]));
      RET(make_lin(c, rp + ".bias_head.fc" + std::to_string(k + 1), &R.bh[k]));
    }
    if (R.wh.back().O != 256 || R.bh.back().O != 1) return fail("HEAD.OUTPUT_DIM must be 256");
    c->has_roienc = true;
  }
  c->host_w.clear();
  c->finalized = true;
  return 0;
}

}  // extern "C"
