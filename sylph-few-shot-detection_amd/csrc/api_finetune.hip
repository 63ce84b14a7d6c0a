// C ABI of the class-code fine-tuning step (include/sylph_hip.h: sylph_fcos_targets, sylph_cls_grad_bytes, sylph_cls_grad): the current
// batch's cls tower output -- a fresh batch's after sylph_fcos_towers or a head entry, or a loaded query record's in place -- read by
// finetune.hip.  Nothing here writes Plan::src, Plan::out, the logits or the decode buffers: a head or a decode that follows finds what
// it would have found without these calls.
#include "api_internal.h"
using namespace sylph_host;

namespace {

// the tower output the streaming kernels read for the current batch, or a refusal that names what is missing
int finetune_src(sylph_ctx* c, const char* who, Plan** P_out, TowerSrc* src) {
  const std::string w(who);
  Plan* P = c->cur;
  if (!P) return fail(w + ": no current batch");
  if (c->dt != DT_BF16)
    return fail(w + ": fine-tuning runs in the bf16 mode only (this context: " + (c->dt == DT_F32S ? "f32s" : "fp32") +
                " storage; there is no fp32 / f32s gradient kernel)");
  if (c->cfg.tower_norm != 0)
    return fail(w + ": MODEL.FCOS.NORM \"none\" is not supported (the gradient kernel reads the cls tower output with its deferred GroupNorm)");
  if (c->cfg.cg_type == 1) return fail(w + ": the ROIEncoder's CondConvBlock (per-class weight scale) is not supported");
  if (c->cfg.cg_code_ksize != 1) return fail(w + ": 3x3 class codes (CODE_GENERATOR.CLS_LAYER kernel size 3) are not supported");
  if (c->rec) {
    if (!c->rec->coef) return fail(w + ": the record holds a normalised tower output (no deferred GroupNorm)");
    src->feat = c->rec->feat; src->coef = c->rec->coef; src->pred = c->rec->pred;
  } else {
    if (!P->head_built || !P->towers_fresh)
      return fail(w + ": the towers have not run on the current batch (call sylph_fcos_towers or a head entry first, or load a query record)");
    if (!P->cls_coef) return fail(w + ": the cls tower's last GroupNorm is not deferred in this build (SYLPH_FUSE_GN_LOGITS=0?)");
    if (P->cls_applied)
      return fail(w + ": an earlier head call on this batch applied the cls tower's last GroupNorm in place; run sylph_fcos_towers again first");
    src->feat = P->cls_feat; src->coef = P->cls_coef; src->pred = P->pred;
  }
  *P_out = P;
  return 0;
}

// the ground truth and the assignment rule of sylph_fcos_targets / sylph_box_samples checked, under the entry's name, and the kernels'
// FcosTargetCfg filled
int fcos_target_cfg(sylph_ctx* c, const std::string& w, int n_gt, const float* boxes_dev, const int* gt_class_dev, const int* gt_image_dev,
                    const float* sizes_of_interest, int n_soi, int center_sample, float pos_radius, FcosTargetCfg* t) {
  if (n_gt < 0) return fail(w + ": n_gt is negative");
  if (n_gt > 0 && (!boxes_dev || !gt_class_dev || !gt_image_dev)) return fail(w + ": a ground-truth array is NULL");
  const int L = c->cfg.nlevels;
  if (!sizes_of_interest || n_soi != L - 1)
    return fail(w + ": sizes_of_interest must hold " + std::to_string(L - 1) + " values (one less than the levels), got " + std::to_string(n_soi));
  if (!(pos_radius > 0.f) && center_sample) return fail(w + ": pos_radius must be positive");
  memset(t, 0, sizeof(*t));
  for (int l = 0; l < L; ++l) {  // fcos_outputs.py:150-160: [-1, s0], [s0, s1], .., [s_last, INF]
    t->strides[l] = c->cfg.strides[l];
    t->lo[l] = l == 0 ? -1.f : sizes_of_interest[l - 1];
    t->hi[l] = l < n_soi ? sizes_of_interest[l] : 100000000.f;
  }
  t->center_sample = center_sample ? 1 : 0;
  t->radius = pos_radius;
  return 0;
}

}  // namespace

/* see include/sylph_hip.h */
int sylph_fcos_targets(sylph_ctx* c, int n_gt, const float* boxes_dev, const int* gt_class_dev, const int* gt_image_dev,
                       const float* sizes_of_interest, int n_soi, int center_sample, float pos_radius, int* labels_out_dev,
                       int* num_pos_out_dev) {
  Plan* P = nullptr;
  TowerSrc src;
  RET(finetune_src(c, "sylph_fcos_targets", &P, &src));
  if (!labels_out_dev || !num_pos_out_dev) return fail("sylph_fcos_targets: an output is NULL");
  FcosTargetCfg t;
  RET(fcos_target_cfg(c, "sylph_fcos_targets", n_gt, boxes_dev, gt_class_dev, gt_image_dev, sizes_of_interest, n_soi, center_sample, pos_radius, &t));
  const int L = c->cfg.nlevels;
  HIPCHK(hipSetDevice(c->device));
  KCHK(launch_fcos_targets(P->head_segs, P->B * L, L, P->hl[0] * P->wl[0], t, n_gt, boxes_dev, gt_class_dev, gt_image_dev, labels_out_dev,
                           num_pos_out_dev, c->stream),
       "fcos_targets");
  return 0;
}

/* see include/sylph_hip.h */
int sylph_cls_grad_bytes(sylph_ctx* c, int N, int64_t* bytes_out) {
  Plan* P = nullptr;
  TowerSrc src;
  RET(finetune_src(c, "sylph_cls_grad_bytes", &P, &src));
  if (N <= 0) return fail("sylph_cls_grad_bytes: class_code is empty");
  if (!bytes_out) return fail("sylph_cls_grad_bytes: bytes_out is NULL");
  *bytes_out = (int64_t)(cls_grad_ws_floats(P->head_mtiles32) * sizeof(float));  // one class block at a time: the blocks of a call share it
  return 0;
}

/* see include/sylph_hip.h */
int sylph_cls_grad(sylph_ctx* c, const int* labels_dev, const float* cls_conv_dev, const float* cls_bias_dev, int N, int class_offset,
                   float alpha, float gamma, void* workspace_dev, float* loss_out_dev, float* grad_w_out_dev, float* grad_b_out_dev) {
  Plan* P = nullptr;
  TowerSrc src;
  RET(finetune_src(c, "sylph_cls_grad", &P, &src));
  if (N <= 0) return fail("sylph_cls_grad: class_code is empty");
  if (class_offset < 0) return fail("sylph_cls_grad: class_offset is negative");
  if (!labels_dev || !cls_conv_dev || !workspace_dev || !loss_out_dev || !grad_w_out_dev) return fail("sylph_cls_grad: a required pointer is NULL");
  if (!(gamma >= 0.f)) return fail("sylph_cls_grad: gamma must not be negative");
  HIPCHK(hipSetDevice(c->device));
  if (!c->ft_codes) {
    RET(ctx_alloc(c, &c->ft_codes, 32 * 256 * sizeof(bf16_t)));
    RET(ctx_alloc(c, (void**)&c->ft_bias, 32 * sizeof(float)));
  }
  const Plan* PP = P;
  for (int n0 = 0; n0 < N; n0 += 32) {
    const int nb = N - n0 < 32 ? N - n0 : 32;
    KCHK(launch_pack_codes(DT_BF16, cls_conv_dev + (size_t)n0 * 256, nb, 256, 32, c->ft_codes, cls_bias_dev ? cls_bias_dev + n0 : nullptr, c->ft_bias,
                           nullptr, c->stream),
         "pack_codes (cls_grad)");
    const double fl = 2.0 * (double)PP->B * PP->Ltot * 32.0 * 256.0 * 3.0;
    KCHK(timed_op(c, "cls_grad_kernel", fl, c->stream,
                  [=](hipStream_t st) {
                    return launch_cls_grad(src.feat, 256, src.coef, c->ft_codes, c->ft_bias, nb, class_offset + n0, labels_dev, alpha, gamma,
                                           (float*)workspace_dev, loss_out_dev, n0 != 0, grad_w_out_dev + (size_t)n0 * 256,
                                           grad_b_out_dev ? grad_b_out_dev + n0 : nullptr, PP->head_segs, PP->head_tiles32, PP->head_mtiles32, st);
                  }),
         "cls_grad");
  }
  return 0;
}

// ---- the box branch: sample bank, loss + gradient, install (box_finetune.hip) ------------------------------------------------------------

namespace {

// what every box-branch entry refuses, by name
int box_mode(sylph_ctx* c, const std::string& w) {
  if (c->dt != DT_BF16)
    return fail(w + ": the box branch is fine-tuned in the bf16 mode only (this context: " + (c->dt == DT_F32S ? "f32s" : "fp32") +
                " storage; there is no fp32 / f32s sample or gradient kernel)");
  if (c->cfg.tower_norm != 0)
    return fail(w + ": MODEL.FCOS.NORM \"none\" is not supported (the samples are cut from the bbox tower output with its deferred GroupNorm)");
  if (c->cfg.cg_type == 1) return fail(w + ": the ROIEncoder is not supported");
  return 0;
}

int grow_ints(sylph_ctx* c, int** p, size_t* cap, size_t need) {
  if (need <= *cap) return 0;
  c->dfree(*p);
  *p = nullptr; *cap = 0;
  RET(ctx_alloc(c, (void**)p, need * sizeof(int)));
  *cap = need;
  return 0;
}

// pred, pred_taps and the biases re-packed from (Cout, 256, 3, 3) / (Cout) into the buffers the cached launches captured, as
// sylph_finalize_weights packs them (api_weights.hip: pack_conv, the tap table)
int install_box_branch(sylph_ctx* c, const std::vector<float>& w, const std::vector<float>& b, const std::vector<float>& scales) {
  const std::vector<uint16_t> pk = pack_conv3x3_bf16(w.data(), c->pred.Cout, c->pred.Cout_pad), tw = pack_pred_taps(w.data(), c->pred.Cout);
  std::vector<float> sh(b);
  sh.resize((size_t)c->pred.Cout_pad, 0.f);
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));  // a queued step may still read the tables
  if (c->side_stream) HIPCHK(hipStreamSynchronize(c->side_stream));
  HIPCHK(hipMemcpy(c->pred.w, pk.data(), pk.size() * 2, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(c->pred.shift, sh.data(), sh.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(c->pred_taps, tw.data(), tw.size() * 2, hipMemcpyHostToDevice));
  c->level_scales = scales;
  c->box_w = w; c->box_b = b;
  // re-packed copies of pred's weights (a prediction conv that went through add_conv) and every cached plan: their segment tables carry
  // SegDesc::mul = the old scales.  The next batch builds its plan again, exactly as a context finalized with these tensors does.
  auto hp = c->hp_weights.find(c->pred.w);
  if (hp != c->hp_weights.end()) { c->dfree(hp->second); c->hp_weights.erase(hp); }
  auto pw = c->pw_weights.find(c->pred.w);
  if (pw != c->pw_weights.end()) { c->dfree(pw->second.first); c->dfree(pw->second.second); c->pw_weights.erase(pw); }
  while (!c->plans.empty()) {
    free_plan(c, c->plans.begin()->second.get());
    c->plans.erase(c->plans.begin());
  }
  c->cur = nullptr;
  c->rec = nullptr;
  return 0;
}

}  // namespace

/* see include/sylph_hip.h */
int sylph_box_samples(sylph_ctx* c, int n_gt, const float* boxes_dev, const int* gt_class_dev, const int* gt_image_dev,
                      const float* sizes_of_interest, int n_soi, int center_sample, float pos_radius, int max_samples, void* patches_out_dev,
                      float* targets_out_dev, int* info_out_dev, int* count_out_dev, int* status_dev) {
  const std::string w = "sylph_box_samples";
  Plan* P = c->cur;
  if (!P) return fail(w + ": no current batch");
  RET(box_mode(c, w));
  if (c->rec)
    return fail(w + ": the current batch is a query record (sylph_record_load): a record holds the cls tower's output and the predictions, no "
                "bbox tower; collect the samples on the fresh batch, after sylph_fcos_towers or a head entry");
  if (!P->head_built || !P->towers_fresh)
    return fail(w + ": the towers have not run on the current batch (call sylph_fcos_towers or a head entry first)");
  const float2* coef = P->tap_coef[1].empty() ? nullptr : P->tap_coef[1].back();
  if (!coef || !c->pred_taps)
    return fail(w + ": the bbox tower's last GroupNorm is not deferred in this build (SYLPH_FUSE_GN_LOGITS=0, or a prediction conv the fused "
                "pass does not take)");
  if (max_samples < 0) return fail(w + ": max_samples is negative");
  if (!count_out_dev || !status_dev || (max_samples > 0 && (!patches_out_dev || !targets_out_dev || !info_out_dev))) return fail(w + ": an output is NULL");
  FcosTargetCfg t;
  RET(fcos_target_cfg(c, w, n_gt, boxes_dev, gt_class_dev, gt_image_dev, sizes_of_interest, n_soi, center_sample, pos_radius, &t));
  const int L = c->cfg.nlevels;
  HIPCHK(hipSetDevice(c->device));
  const int max_rows = P->hl[0] * P->wl[0], nseg = P->B * L;
  RET(grow_ints(c, &c->bx_assign, &c->bx_assign_cap, (size_t)P->B * P->Ltot));
  RET(grow_ints(c, &c->bx_blk, &c->bx_blk_cap, (size_t)nseg * box_samples_gx(max_rows)));
  const void* x = P->tap_out[1].back();
  const Plan* PP = P;
  KCHK(timed_op(c, "box_samples", 0.0, c->stream,
                [=](hipStream_t st) {
                  return launch_box_samples(x, coef, PP->head_segs, nseg, L, max_rows, PP->Ltot, t, n_gt, boxes_dev, gt_class_dev, gt_image_dev,
                                            c->bx_assign, c->bx_blk, max_samples, patches_out_dev, targets_out_dev, info_out_dev, count_out_dev,
                                            status_dev, st);
                }),
       "box_samples");
  return 0;
}

/* see include/sylph_hip.h */
int sylph_box_grad_bytes(sylph_ctx* c, int n, int64_t* bytes_out) {
  RET(box_mode(c, "sylph_box_grad_bytes"));
  if (n < 0) return fail("sylph_box_grad_bytes: n is negative");
  if (!bytes_out) return fail("sylph_box_grad_bytes: bytes_out is NULL");
  *bytes_out = (int64_t)(box_grad_ws_floats(n) * sizeof(float));
  return 0;
}

/* see include/sylph_hip.h */
int sylph_box_grad(sylph_ctx* c, int n, const void* patches_dev, const float* targets_dev, const int* info_dev, const float* w_dev,
                   const float* b_dev, const float* scales_dev, int quality, int iou_mask, void* workspace_dev, float* sums_out_dev,
                   float* grad_w_out_dev, float* grad_b_out_dev, float* grad_scales_out_dev, float* z_out_dev, float* g_out_dev) {
  const std::string w = "sylph_box_grad";
  RET(box_mode(c, w));
  if (!c->finalized || !c->has_head) return fail(w + ": FCOS head weights were not loaded");
  const int cout = c->pred.Cout;
  if (c->pred.KH != 3 || c->pred.Cin != 256 || cout < 5 || cout > 6)
    return fail(w + ": the box branch must be a 3x3 conv of 256 -> 5 or 6 channels (bbox_pred + ctrness [+ iou_overlap]); this context has " +
                std::to_string(cout));
  if (n < 0) return fail(w + ": n is negative");
  if (quality < 1 || quality > 3) return fail(w + ": quality must be 1 (ctrness), 2 (iou) or 3 (both), got " + std::to_string(quality));
  if ((quality & 2) && cout < 6) return fail(w + ": BOX_QUALITY names \"iou\" but the context has no iou_overlap channel");
  if (n > 0 && (!patches_dev || !targets_dev || !info_dev || !workspace_dev)) return fail(w + ": a required pointer is NULL");
  if (!w_dev || !b_dev || !scales_dev || !sums_out_dev || !grad_w_out_dev || !grad_b_out_dev || !grad_scales_out_dev)
    return fail(w + ": a required pointer is NULL");
  HIPCHK(hipSetDevice(c->device));
  const int L = c->cfg.nlevels;
  const double fl = 2.0 * (double)n * 2304.0 * cout * 2.0;
  KCHK(timed_op(c, "box_grad_kernel", fl, c->stream,
                [=](hipStream_t st) {
                  return launch_box_grad(n, patches_dev, targets_dev, info_dev, w_dev, b_dev, scales_dev, cout, L, quality, iou_mask ? 1 : 0,
                                         (float*)workspace_dev, sums_out_dev, grad_w_out_dev, grad_b_out_dev, grad_scales_out_dev, z_out_dev,
                                         g_out_dev, st);
                }),
       "box_grad");
  return 0;
}

/* see include/sylph_hip.h */
int sylph_box_branch_shape(sylph_ctx* c, int* cout, int* nlevels, uint64_t* stamp) {
  if (!c->finalized || !c->has_head || c->box_w.empty()) return fail("sylph_box_branch_shape: no 3x3 box branch is loaded");
  if (cout) *cout = c->pred.Cout;
  if (nlevels) *nlevels = c->cfg.nlevels;
  if (stamp) *stamp = c->box_stamp;
  return 0;
}

/* see include/sylph_hip.h */
int sylph_get_box_branch(sylph_ctx* c, float* w_host, float* b_host, float* scales_host) {
  if (!c->finalized || !c->has_head || c->box_w.empty()) return fail("sylph_get_box_branch: no 3x3 box branch is loaded");
  if (w_host) memcpy(w_host, c->box_w.data(), c->box_w.size() * sizeof(float));
  if (b_host) memcpy(b_host, c->box_b.data(), c->box_b.size() * sizeof(float));
  if (scales_host) memcpy(scales_host, c->level_scales.data(), c->level_scales.size() * sizeof(float));
  return 0;
}

/* see include/sylph_hip.h */
int sylph_set_box_branch(sylph_ctx* c, const float* w_host, const float* b_host, const float* scales_host) {
  const std::string w = "sylph_set_box_branch";
  if (!c->finalized || !c->has_head || c->box_w.empty()) return fail(w + ": no 3x3 box branch is loaded");
  RET(box_mode(c, w));
  if (!c->pred_taps) return fail(w + ": this context has no fused prediction pass (pred_taps): the box branch cannot be replaced");
  const bool none = !w_host && !b_host && !scales_host;
  if (!none && (!w_host || !b_host || !scales_host)) return fail(w + ": pass the three tensors, or three NULLs to restore the finalized ones");
  if (none) {
    if (c->box_stamp == 0) return 0;
    RET(install_box_branch(c, c->box_w0, c->box_b0, c->box_s0));
    c->box_stamp = 0;
    return 0;
  }
  const size_t L = (size_t)c->cfg.nlevels;
  std::vector<float> sc(scales_host, scales_host + L);
  if (!c->cfg.use_scale)
    for (float v : sc)
      if (v != 1.f) return fail(w + ": MODEL.FCOS.USE_SCALE is off: every scale must be 1");
  RET(install_box_branch(c, std::vector<float>(w_host, w_host + c->box_w0.size()), std::vector<float>(b_host, b_host + c->box_b0.size()), sc));
  c->box_stamp = ++c->box_stamp_next;
  return 0;
}
