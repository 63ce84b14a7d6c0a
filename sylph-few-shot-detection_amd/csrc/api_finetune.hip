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

}  // namespace

/* see include/sylph_hip.h */
int sylph_fcos_targets(sylph_ctx* c, int n_gt, const float* boxes_dev, const int* gt_class_dev, const int* gt_image_dev,
                       const float* sizes_of_interest, int n_soi, int center_sample, float pos_radius, int* labels_out_dev,
                       int* num_pos_out_dev) {
  Plan* P = nullptr;
  TowerSrc src;
  RET(finetune_src(c, "sylph_fcos_targets", &P, &src));
  if (n_gt < 0) return fail("sylph_fcos_targets: n_gt is negative");
  if (n_gt > 0 && (!boxes_dev || !gt_class_dev || !gt_image_dev)) return fail("sylph_fcos_targets: a ground-truth array is NULL");
  if (!labels_out_dev || !num_pos_out_dev) return fail("sylph_fcos_targets: an output is NULL");
  const int L = c->cfg.nlevels;
  if (!sizes_of_interest || n_soi != L - 1)
    return fail("sylph_fcos_targets: sizes_of_interest must hold " + std::to_string(L - 1) + " values (one less than the levels), got " + std::to_string(n_soi));
  if (!(pos_radius > 0.f) && center_sample) return fail("sylph_fcos_targets: pos_radius must be positive");
  FcosTargetCfg t;
  memset(&t, 0, sizeof(t));
  for (int l = 0; l < L; ++l) {  // fcos_outputs.py:150-160: [-1, s0], [s0, s1], .., [s_last, INF]
    t.strides[l] = c->cfg.strides[l];
    t.lo[l] = l == 0 ? -1.f : sizes_of_interest[l - 1];
    t.hi[l] = l < n_soi ? sizes_of_interest[l] : 100000000.f;
  }
  t.center_sample = center_sample ? 1 : 0;
  t.radius = pos_radius;
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
    Plan* owner = c->alloc_owner;
    c->alloc_owner = nullptr;  // the context's: plan eviction must not free it
    int r = c->dalloc(&c->ft_codes, 32 * 256 * sizeof(bf16_t));
    if (r == 0) r = c->dalloc((void**)&c->ft_bias, 32 * sizeof(float));
    c->alloc_owner = owner;
    RET(r);
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
