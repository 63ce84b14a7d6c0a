// C ABI of the code generator's meta-training step (include/sylph_hip.h: sylph_codegen_param_layout, sylph_codegen_train_bytes,
// sylph_codegen_train_shape, sylph_codegen_train_forward, sylph_codegen_train_backward): the host checks in front of codegen_train.hip.
// Neither entry needs a current batch, and nothing here touches a plan, a record or the serving weights.
#include "api_internal.h"
using namespace sylph_host;

namespace {

// the kernel-side description of the generator, or why this config cannot be trained
bool trainable_cfg(const sylph_ctx* c, CgtCfg* g, std::string* why) {
  if (c->cfg.cg_type == 1) { *why = "the ROIEncoder is not supported (CodeGenerator heads only)"; return false; }
  if (c->cfg.cg_code_ksize != 1) { *why = "3x3 class codes (CODE_GENERATOR.CLS_LAYER kernel size 3) are not supported"; return false; }
  if (c->cfg.cg_has_weight) { *why = "CODE_GENERATOR.WEIGHT_LAYER heads are not supported"; return false; }
  if (c->cfg.cg_has_scale) { *why = "CODE_GENERATOR.SCALE_LAYER heads are not supported"; return false; }
  if (c->cfg.cg_bias_l2_norm) { *why = "CODE_GENERATOR.BIAS_L2_NORM is not supported"; return false; }
  if (c->cfg.cg_meta_bias) { *why = "CODE_GENERATOR.META_BIAS (a learned bias_value) is not supported"; return false; }
  const int L = c->cfg.cg_tower_layers;
  if (L < 0 || L > CGT_MAX_TOWER) {
    *why = "CODE_GENERATOR.TOWER_LAYERS has " + std::to_string(L) + " entries; at most " + std::to_string(CGT_MAX_TOWER);
    return false;
  }
  for (int i = 0; i < L; ++i)
    if (!((c->cfg.cg_tower_gn_mask >> i) & 1) || !((c->cfg.cg_tower_relu_mask >> i) & 1)) {
      *why = "CODE_GENERATOR.TOWER_LAYERS[" + std::to_string(i) + "] is not [\"GN\", \"ReLU\"]; no other tower entry is supported";
      return false;
    }
  g->L = L;
  g->has_bias = c->cfg.cg_has_bias ? 1 : 0;
  g->post_norm = c->cfg.cg_post_norm ? 1 : 0;
  g->l2_norm = c->cfg.cg_conv_l2_norm ? 1 : 0;
  g->has_conv_scale = (c->cfg.cg_use_weight_scale && (c->cfg.cg_conv_l2_norm || c->cfg.cg_post_norm)) ? 1 : 0;
  g->prior = -logf((1.f - c->cfg.prior_prob) / c->cfg.prior_prob);
  return true;
}

// what every entry refuses, by name
int train_mode(sylph_ctx* c, const std::string& w, CgtCfg* g) {
  if (c->dt != DT_BF16)
    return fail(w + ": the code generator is trained in the bf16 mode only (this context: " + (c->dt == DT_F32S ? "f32s" : "fp32") +
                " storage; there is no fp32 / f32s training kernel)");
  std::string why;
  if (!trainable_cfg(c, g, &why)) return fail(w + ": " + why);
  return 0;
}

int check_sizes(const std::string& w, int n_rows, int M, int n_seg) {
  if (n_rows < 1) return fail(w + ": n_rows = " + std::to_string(n_rows) + " (the ROI bank is empty)");
  if (M < 1) return fail(w + ": M = " + std::to_string(M) + " (at least one index is needed)");
  if (n_seg < 1) return fail(w + ": n_seg = " + std::to_string(n_seg) + " (at least one segment is needed)");
  if ((long)M * 49 * 256 > 0x7fffffffL) return fail(w + ": M = " + std::to_string(M) + " shots in one step; at most 171196");
  return 0;
}

}  // namespace

namespace sylph_host {

// (state-dict key, offset, element count) of every trainable tensor, in the order of the flat vector
void codegen_layout_entries(const CgtCfg& g, std::vector<std::string>* keys, std::vector<int64_t>* off, std::vector<int64_t>* cnt) {
  CgtParams P;
  cgt_param_layout(g, &P);
  const std::string cp = "code_generator.code_generator_head";
  auto add = [&](const std::string& k, long o, int64_t n) {
    if (o < 0) return;
    keys->push_back(cp + k); off->push_back(o); cnt->push_back(n);
  };
  for (int i = 0; i < g.L; ++i) {  // nn.Sequential: conv 3 i, GroupNorm 3 i + 1, ReLU 3 i + 2 (code_generator.py:648-688)
    const std::string t = ".support_set_shared_tower.";
    add(t + std::to_string(3 * i) + ".weight", P.tw[i], 256 * 2304);
    add(t + std::to_string(3 * i) + ".bias", P.tb[i], 256);
    add(t + std::to_string(3 * i + 1) + ".weight", P.tg[i], 256);
    add(t + std::to_string(3 * i + 1) + ".bias", P.tbe[i], 256);
  }
  add(".support_set_cls_conv.0.weight", P.cw, 256 * 2304);
  add(".support_set_cls_conv.0.bias", P.cb, 256);
  add(".support_set_cls_bias.0.weight", P.bw, 2304);
  add(".support_set_cls_bias.0.bias", P.bb, 1);
  add(".post_norm.weight", P.pg, 256);
  add(".post_norm.bias", P.pb, 256);
  add(".conv_scale.scale", P.cs, 1);
  add(".bias_scale.scale", P.bs, 1);
}


// sylph_finalize_weights: the generator as loaded, in the flat layout (what sylph_get_code_generator returns and a restore installs);
// nothing when the config has no trainable layout
void capture_code_generator(sylph_ctx* c) {
  c->cg_flat0.clear(); c->cg_flat.clear();
  c->cg_stamp = 0;
  CgtCfg g;
  std::string why;
  if (!trainable_cfg(c, &g, &why)) return;
  std::vector<std::string> keys;
  std::vector<int64_t> off, cnt;
  codegen_layout_entries(g, &keys, &off, &cnt);
  std::vector<float> flat((size_t)(off.back() + cnt.back()), 0.f);
  for (size_t i = 0; i < keys.size(); ++i) {
    const HostTensor* t = find_w(c, keys[i]);
    if (!t || (int64_t)t->data.size() != cnt[i]) return;
    std::copy(t->data.begin(), t->data.end(), flat.begin() + off[i]);
  }
  c->cg_flat0 = flat;
  c->cg_flat = flat;
}

}  // namespace sylph_host

namespace {

// The support convolutions, GroupNorm tables and tail constants re-packed from the flat vector INTO the device buffers the cached support
// passes captured, as sylph_finalize_weights packs them (api_weights.hip: pack_conv, make_conv_bias, make_gn); conv_hpipe's re-packed
// copy of a layer, where one exists, is packed again in place.  Every cached pass therefore runs the new generator from its next call on.
int install_code_generator(sylph_ctx* c, const CgtCfg& g, const std::vector<float>& flat) {
  CgtParams P;
  cgt_param_layout(g, &P);
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));  // a queued support pass may still read the tables
  if (c->side_stream) HIPCHK(hipStreamSynchronize(c->side_stream));
  auto put_conv = [&](ConvLayer& L, long wo, long bo, int cout) -> int {
    if (L.KH != 3 || L.KW != 3 || L.Cin != 256 || L.Cout != cout || !L.w || !L.shift) return fail("sylph_set_code_generator: internal: unexpected support conv");
    const std::vector<uint16_t> pk = pack_conv3x3_bf16(flat.data() + wo, cout, L.Cout_pad);
    std::vector<float> sh((size_t)L.Cout_pad, 0.f);
    std::copy(flat.begin() + bo, flat.begin() + bo + cout, sh.begin());
    HIPCHK(hipMemcpy(L.w, pk.data(), pk.size() * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(L.shift, sh.data(), sh.size() * 4, hipMemcpyHostToDevice));
    auto hp = c->hp_weights.find(L.w);
    if (hp != c->hp_weights.end()) {
      KCHK(launch_hpipe_pack_weights(L.w, hp->second, L.Cout, L.Cin, c->stream), "hpipe_pack_weights");
      HIPCHK(hipStreamSynchronize(c->stream));
    }
    return 0;
  };
  auto put_gn = [&](GNLayer& G, long go, long bo) -> int {
    HIPCHK(hipMemcpy(G.gamma, flat.data() + go, 256 * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(G.beta, flat.data() + bo, 256 * 4, hipMemcpyHostToDevice));
    return 0;
  };
  for (int i = 0; i < g.L; ++i) {
    RET(put_conv(c->cg_tower[i], P.tw[i], P.tb[i], 256));
    RET(put_gn(c->cg_gn[i], P.tg[i], P.tbe[i]));
  }
  RET(put_conv(c->cg_cls, P.cw, P.cb, 256));
  if (g.has_bias) RET(put_conv(c->cg_bias, P.bw, P.bb, 1));
  if (g.post_norm) RET(put_gn(c->cg_post, P.pg, P.pb));
  c->cg_conv_scale = P.cs >= 0 ? flat[P.cs] : 1.f;
  c->cg_bias_scale = P.bs >= 0 ? flat[P.bs] : 1.f;
  c->cg_flat = flat;
  return 0;
}

}  // namespace

/* see include/sylph_hip.h */
int sylph_get_code_generator(sylph_ctx* c, float* flat_host) {
  CgtCfg g;
  RET(train_mode(c, "sylph_get_code_generator", &g));
  if (!c->has_codegen || c->cg_flat0.empty()) return fail("sylph_get_code_generator: code generator weights were not loaded");
  if (!flat_host) return fail("sylph_get_code_generator: flat_host is NULL");
  memcpy(flat_host, c->cg_flat0.data(), c->cg_flat0.size() * sizeof(float));
  return 0;
}

/* see include/sylph_hip.h */
int sylph_set_code_generator(sylph_ctx* c, const float* flat_host) {
  const std::string w = "sylph_set_code_generator";
  CgtCfg g;
  RET(train_mode(c, w, &g));
  if (!c->has_codegen || c->cg_flat0.empty()) return fail(w + ": code generator weights were not loaded");
  if (!flat_host) {
    if (c->cg_stamp == 0) return 0;
    RET(install_code_generator(c, g, c->cg_flat0));
    c->cg_stamp = 0;
    return 0;
  }
  RET(install_code_generator(c, g, std::vector<float>(flat_host, flat_host + c->cg_flat0.size())));
  c->cg_stamp = ++c->cg_stamp_next;
  return 0;
}

/* see include/sylph_hip.h */
int sylph_codegen_stamp(sylph_ctx* c, uint64_t* stamp) {
  if (!stamp) return fail("sylph_codegen_stamp: stamp is NULL");
  *stamp = c->cg_stamp;
  return 0;
}

/* see include/sylph_hip.h */
int sylph_codegen_param_layout(sylph_ctx* c, int max_entries, char* keys_out, int64_t* offset_out, int64_t* numel_out, int* n_out,
                               int64_t* total_out) {
  CgtCfg g;
  RET(train_mode(c, "sylph_codegen_param_layout", &g));
  std::vector<std::string> keys;
  std::vector<int64_t> off, cnt;
  codegen_layout_entries(g, &keys, &off, &cnt);
  if (n_out) *n_out = (int)keys.size();
  if (total_out) *total_out = off.back() + cnt.back();
  if (!keys_out && !offset_out && !numel_out) return 0;
  if (max_entries < (int)keys.size())
    return fail("sylph_codegen_param_layout: " + std::to_string(keys.size()) + " tensors, room for " + std::to_string(max_entries));
  for (size_t i = 0; i < keys.size(); ++i) {
    if (keys_out) snprintf(keys_out + 128 * i, 128, "%s", keys[i].c_str());
    if (offset_out) offset_out[i] = off[i];
    if (numel_out) numel_out[i] = cnt[i];
  }
  return 0;
}

/* see include/sylph_hip.h */
int sylph_codegen_train_bytes(sylph_ctx* c, int M, int n_seg, int64_t* bytes_out) {
  const std::string w = "sylph_codegen_train_bytes";
  CgtCfg g;
  RET(train_mode(c, w, &g));
  RET(check_sizes(w, 1, M, n_seg));
  if (!bytes_out) return fail(w + ": bytes_out is NULL");
  CgtWs W;
  cgt_workspace(g, M, n_seg, &W);
  *bytes_out = (int64_t)W.total;
  return 0;
}

/* see include/sylph_hip.h */
int sylph_codegen_train_shape(sylph_ctx* c, int M, int n_seg, int* units_out, int* passes_out, int64_t* debug_floats_out) {
  const std::string w = "sylph_codegen_train_shape";
  CgtCfg g;
  RET(train_mode(c, w, &g));
  RET(check_sizes(w, 1, M, n_seg));
  CgtWs W;
  cgt_workspace(g, M, n_seg, &W);
  if (units_out) *units_out = W.units;
  if (passes_out) *passes_out = W.passes;
  if (debug_floats_out) *debug_floats_out = (int64_t)cgt_debug_floats(g, M, n_seg);
  return 0;
}

/* see include/sylph_hip.h */
int sylph_codegen_train_forward(sylph_ctx* c, const float* params_dev, const void* rows_dev, int n_rows, int M, const int* idx, int n_seg,
                                const int* seg_len, void* workspace_dev, float* codes_out_dev) {
  const std::string w = "sylph_codegen_train_forward";
  CgtCfg g;
  RET(train_mode(c, w, &g));
  RET(check_sizes(w, n_rows, M, n_seg));
  if (!params_dev || !rows_dev || !idx || !seg_len || !workspace_dev || !codes_out_dev) return fail(w + ": a required pointer is NULL");
  for (int i = 0; i < M; ++i)
    if (idx[i] < 0 || idx[i] >= n_rows)
      return fail(w + ": idx[" + std::to_string(i) + "] = " + std::to_string(idx[i]) + " is outside the bank of " + std::to_string(n_rows) + " rows");
  long total = 0;
  for (int j = 0; j < n_seg; ++j) {
    if (seg_len[j] < 1) return fail(w + ": seg_len[" + std::to_string(j) + "] = " + std::to_string(seg_len[j]) + " (a segment needs at least one shot)");
    total += seg_len[j];
  }
  if (total != M) return fail(w + ": the segment lengths sum to " + std::to_string(total) + ", not to M = " + std::to_string(M));
  CgtWs W;
  cgt_workspace(g, M, n_seg, &W);
  std::vector<int> seg(2 * (size_t)n_seg);
  for (int j = 0, i0 = 0; j < n_seg; i0 += seg_len[j], ++j) { seg[2 * j] = i0; seg[2 * j + 1] = seg_len[j]; }
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));  // an earlier step may still read the tables of this workspace
  HIPCHK(hipMemcpy((char*)workspace_dev + W.idx, idx, (size_t)M * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy((char*)workspace_dev + W.seg, seg.data(), seg.size() * sizeof(int), hipMemcpyHostToDevice));
  c->cgt_ws = nullptr;
  const double fl = 2.0 * (double)M * 49.0 * 2304.0 * 256.0 * g.L + 2.0 * (double)M * 2304.0 * 257.0;
  KCHK(timed_op(c, "codegen_train_forward", fl, c->stream,
                [=](hipStream_t st) { return launch_cgt_forward(g, params_dev, rows_dev, M, n_seg, (char*)workspace_dev, codes_out_dev, st); }),
       "codegen_train_forward");
  c->cgt_ws = workspace_dev; c->cgt_M = M; c->cgt_nseg = n_seg; c->cgt_rows = n_rows;
  return 0;
}

/* see include/sylph_hip.h */
int sylph_codegen_train_backward(sylph_ctx* c, const float* params_dev, const void* rows_dev, int n_rows, int M, int n_seg, void* workspace_dev,
                                 const float* grad_codes_dev, float* grad_out_dev, float* debug_out_dev) {
  const std::string w = "sylph_codegen_train_backward";
  CgtCfg g;
  RET(train_mode(c, w, &g));
  RET(check_sizes(w, n_rows, M, n_seg));
  if (!params_dev || !rows_dev || !workspace_dev || !grad_codes_dev || !grad_out_dev) return fail(w + ": a required pointer is NULL");
  if (!c->cgt_ws || c->cgt_ws != workspace_dev || c->cgt_M != M || c->cgt_nseg != n_seg || c->cgt_rows != n_rows)
    return fail(w + ": the workspace does not hold the preceding sylph_codegen_train_forward of this episode (same workspace, n_rows, M and n_seg)");
  HIPCHK(hipSetDevice(c->device));
  const double fl = 2.0 * (double)M * 49.0 * 2304.0 * 256.0 * (g.L + (g.L > 0 ? g.L - 1 : 0)) + 4.0 * (double)M * 2304.0 * 257.0;
  KCHK(timed_op(c, "codegen_train_backward", fl, c->stream,
                [=](hipStream_t st) {
                  return launch_cgt_backward(g, params_dev, rows_dev, M, n_seg, (char*)workspace_dev, grad_codes_dev, grad_out_dev, debug_out_dev, st);
                }),
       "codegen_train_backward");
  return 0;
}
