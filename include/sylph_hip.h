/* libsylph_hip.so -- C ABI of the MI355X-native Sylph few-shot detection inference path.
 *
 * The reference (facebookresearch/sylph-few-shot-detection) is 100 % Python and has no FFI: its
 * "ABI" for this path is nn.Module.forward.  Each entry point below names the reference call it
 * replaces (paths relative to the reference root).  Plain pointers and sizes only; device pointers
 * are raw HIP device addresses (e.g. torch.Tensor.data_ptr()), the caller owns every buffer it
 * passes in, the library owns only the weights and workspace held by the context.
 *
 * Conventions
 *   - return value: 0 on success, non-zero on error; sylph_last_error() gives the message.
 *   - one context per process / GPU (the reference runs one process per GPU,
 *     tools/train_net.py:98-106); kernels are enqueued on the stream given to sylph_set_stream
 *     (default: the NULL stream).  No internal threads.  Calls do not synchronise unless stated.
 *   - "current batch": sylph_preprocess / sylph_import_pyramid select the batch (B, H, W) the
 *     following stage calls operate on.
 */
#ifndef SYLPH_HIP_H
#define SYLPH_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sylph_ctx sylph_ctx;

enum { SYLPH_F32 = 0, SYLPH_BF16 = 1, SYLPH_F32S = 2 };

/* Subset of the yacs config the path reads (sylph/runner/adet_configs.py:25-61,
 * sylph/runner/default_configs.py:43-167). */
typedef struct sylph_config {
  int resnet_depth;        /* MODEL.RESNETS.DEPTH: 50 | 101 | 152 (bottleneck blocks, stage widths 256 << s), 18 | 34 (BasicBlock,
                              stage widths 64 << s = RES2_OUT_CHANNELS 64; needs num_groups 1, width_per_group 64; stride_in_1x1 is ignored) */
  int stride_in_1x1;       /* MODEL.RESNETS.STRIDE_IN_1X1 */
  int num_cls_convs;       /* MODEL.FCOS.NUM_CLS_CONVS */
  int num_box_convs;       /* MODEL.FCOS.NUM_BOX_CONVS */
  int nlevels;             /* len(MODEL.FCOS.FPN_STRIDES) == 5 */
  int strides[8];          /* MODEL.FCOS.FPN_STRIDES */
  float pixel_mean[3];     /* MODEL.PIXEL_MEAN */
  float pixel_std[3];      /* MODEL.PIXEL_STD */
  int size_divisibility;   /* backbone.size_divisibility (32) */
  int use_scale;           /* MODEL.FCOS.USE_SCALE */
  int cond_use_bias;       /* MODEL.META_LEARN.CODE_GENERATOR.USE_BIAS (CondConvBasic use_bias) */
  float pre_nms_thresh;    /* MODEL.FCOS.INFERENCE_TH_TEST */
  int pre_nms_topk;        /* MODEL.FCOS.PRE_NMS_TOPK_TEST */
  float nms_thresh;        /* MODEL.FCOS.NMS_TH */
  int post_nms_topk;       /* MODEL.FCOS.POST_NMS_TOPK_TEST */
  int thresh_with_ctr;     /* MODEL.FCOS.THRESH_WITH_CTR */
  int quality_mode;        /* MODEL.FCOS.BOX_QUALITY: 0 ["ctrness"], 1 ["iou"], 2 ["ctrness","iou"] */
  int cg_tower_layers;     /* len(CODE_GENERATOR.TOWER_LAYERS) (each ["GN","ReLU"]) */
  int cg_has_bias;         /* len(CODE_GENERATOR.BIAS_LAYER) != 0 */
  int cg_bias_l2_norm;     /* CODE_GENERATOR.BIAS_L2_NORM */
  int cg_post_norm;        /* CODE_GENERATOR.POST_NORM == "GN" */
  int cg_conv_l2_norm;     /* CODE_GENERATOR.CONV_L2_NORM */
  int cg_use_weight_scale; /* CODE_GENERATOR.USE_WEIGHT_SCALE */
  float prior_prob;        /* MODEL.FCOS.PRIOR_PROB */
  int cand_cap;            /* per (image, level) candidate capacity of the decode scan (0 = default: every location x class score of the largest level up to 262144 slots, else 1/8 of them, at most 4 M) */
  /* ROIEncoder variant (sylph/runner/default_configs.py:149-167; LVIS ROI-Encoder yaml) */
  int cg_type;             /* CODE_GENERATOR.NAME: 0 "CodeGenerator", 1 "ROIEncoder" */
  int tok_num_conv;        /* TOKENIZER.NUM_CONV (conv3x3 + GN + ReLU, CONV_DIM 256, NORM "GN") */
  int tok_num_fc;          /* TOKENIZER.NUM_FC (FC_DIM 256) */
  int enc_layers;          /* TRANSFORMER_ENCODER.LAYERS */
  int head_num_fc;         /* HEAD.NUM_FC */
  int head_fc_dim;         /* HEAD.FC_DIM (OUTPUT_DIM 256) */
  int cg_meta_bias;        /* CODE_GENERATOR.META_BIAS: the bias prior is the learned parameter
                              code_generator.code_generator_head.bias_value of the checkpoint (code_generator.py:422-425,856) */
  int cg_has_weight;       /* len(CODE_GENERATOR.WEIGHT_LAYER) != 0: learned per-shot weights, softmax over the shots of a class
                              (support_set_cls_weight: conv3x3 256->1 + global average pool; code_generator.py:583-613,766-777) */
  int cg_has_scale;        /* len(CODE_GENERATOR.SCALE_LAYER) != 0: per-class weight norm "cls_weight_norm"
                              (support_set_cls_scale: conv3x3 256->1 + global average pool; code_generator.py:615-645,976-993) */
  int num_share_convs;     /* MODEL.FCOS.NUM_SHARE_CONVS: layers of the shared tower in front of the cls / bbox towers (fcos.py:397,626) */
  int tower_norm;          /* MODEL.FCOS.NORM: 0 "GN" (and "NaiveGN": adet's NaiveGroupNorm is the same arithmetic), 1 "none": the
                              towers are (conv3x3 + bias, ReLU) x n, nn.Sequential conv index 2 i instead of 3 i (fcos.py:72-122,399) */
  int cg_tower_gn_mask;    /* CODE_GENERATOR.TOWER_LAYERS[i][0] == "GN"   -> bit i (sylph_config_default: all ones = ["GN", "ReLU"] layers); */
  int cg_tower_relu_mask;  /* CODE_GENERATOR.TOWER_LAYERS[i][1] == "ReLU" -> bit i.  A layer without norm / activation has no such module
                              in support_set_shared_tower, whose nn.Sequential indices advance per EXISTING module (code_generator.py:648-688) */
  int tower_deformable;    /* MODEL.FCOS.USE_DEFORMABLE: the LAST conv of the cls and of the bbox tower is a modulated deformable conv (adet
                              DFConv2d, DCNv2): keys {k}.offset.weight / .bias [27,256,3,3] and {k}.conv.weight / .bias instead of {k}.weight
                              / .bias (fcos.py:83-84). */
  int num_groups;          /* MODEL.RESNETS.NUM_GROUPS: groups of every bottleneck's 3x3 conv2 (1 = ResNet, > 1 = ResNeXt) */
  int width_per_group;     /* MODEL.RESNETS.WIDTH_PER_GROUP: conv2 channels per group in res2 (doubling per stage); the bottleneck width of
                              stage s (0 = res2) is num_groups * width_per_group << s (detectron2 build_resnet_backbone) */
  int mobilenet;           /* MODEL.MOBILENET: the bottom-up path is AdelaiDet's MobileNetV2 (adet/modeling/backbone/mobilenet.py, width 1.0,
                              FrozenBN): keys backbone.bottom_up.features.{0..17}.*, res2..res5 = the outputs of features 3 / 6 / 13 / 17
                              with 24 / 32 / 96 / 320 channels; the FPN laterals read 32 / 96 / 320 channels.  MODEL.RESNETS.* is not read. */
  int cg_code_ksize;       /* CODE_GENERATOR.CLS_LAYER[2]: spatial size k of a class code, 1 or 3 (GlobalAdaptiveAvgPool2d(k_s = k),
                              code_generator.py:519-540).  A code row is 256 k^2 + 1 floats: cls_conv.reshape(-1) in (c, ky, kx) order,
                              then the bias; the query head runs it as a k x k conv with padding k / 2 (fcos.py:499-510,
                              head_utils.py:60-81).  The ROIEncoder (cg_type 1) ignores it (fcos.py:524): its codes stay 1x1. */
} sylph_config;

/* Fill cfg with the defaults of the COCO Meta-FCOS finetune yaml. */
void sylph_config_default(sylph_config* cfg);

/* Context.  dtype = SYLPH_BF16 (bf16 storage + MFMA, fp32 accumulate: the throughput mode), SYLPH_F32 (exact-fp32 MFMA: the reference
 * arithmetic, fcos_outputs.py:904-1028 within 1e-3 with identical NMS indices) or SYLPH_F32S (the parity mode at speed: fp32 storage
 * everywhere as in SYLPH_F32, every conv product as three bf16 MFMAs on operands split into bf16 hi + lo parts -- 2^-17 relative per
 * operand, the same 1e-3 bound). */
int sylph_ctx_create(int device_id, int dtype, sylph_ctx** out);
void sylph_ctx_destroy(sylph_ctx* ctx);
const char* sylph_last_error(void);
int sylph_set_stream(sylph_ctx* ctx, void* hip_stream);
int sylph_set_config(sylph_ctx* ctx, const sylph_config* cfg);

/* Weights: replaces DetectionCheckpointer(model).load (sylph/predictor.py:87-88).  name is the
 * reference state-dict key, data is host fp32 in the reference's tensor layout.
 * sylph_finalize_weights packs them for the kernels (K-major bf16/fp32, folded FrozenBN). */
int sylph_load_weight(sylph_ctx* ctx, const char* name, const float* data_host, const int64_t* shape, int ndim);
int sylph_finalize_weights(sylph_ctx* ctx);

/* MetaProposalNetwork.convert_batched_inputs_to_image_list
 * (sylph/modeling/meta_arch/meta_one_stage_detector.py:174-178): B device images, each (3,h,w) fp32
 * BGR 0-255 -> normalised, zero padded to a common size divisible by size_divisibility.
 * Host arrays: images_dev[B], heights[B], widths[B].  Returns the padded size.
 * bf16 mode: the normalisation is applied by the stem kernel of the next sylph_backbone_fpn call on the way into its LDS patch (same
 * arithmetic, bit-identical; no normalised copy of the batch is written) -- the images must stay valid and unchanged until that call
 * has been enqueued, on the same stream.  SYLPH_FUSE_PREPROCESS=0: a separate pass here. */
int sylph_preprocess(sylph_ctx* ctx, int B, const float* const* images_dev, const int* heights, const int* widths,
                     int* padded_h, int* padded_w);

/* Fused input pipeline: what SylphPredictor does on the host before the model call
 * (sylph/predictor.py:117-120,259-269: detectron2 ResizeShortestEdge -> ResizeTransform = PIL BILINEAR on the uint8 image,
 * RGB->BGR when INPUT.FORMAT is RGB, float CHW tensor) fused with convert_batched_inputs_to_image_list.  images_dev[b]:
 * device pointer to a (h, w, 3) uint8 HWC image (e.g. copied from a pinned host batch); new_heights/new_widths: the resize
 * targets.  Pillow's fixed-point two-pass resampling is reproduced bit for bit.  Makes the padded batch current. */
int sylph_preprocess_u8(sylph_ctx* ctx, int B, const unsigned char* const* images_dev, const int* heights, const int* widths,
                        const int* new_heights, const int* new_widths, int rgb_input, int* padded_h, int* padded_w);
/* The same pipeline for VIEWS of device-resident sources (test-time augmentation, tiled inference): image b of the batch is built from
 * the (src_h[b], src_w[b], 3) uint8 HWC image at src_dev[b] as Image.fromarray(src).crop((x0, y0, x0 + cw, y0 + ch))
 * .resize((new_w, new_h), BILINEAR), then ImageOps.mirror of that result when flip[b] != 0 (detectron2's transform list puts the flip
 * behind the resize), then BGR swap, normalisation and padding -- bit for bit what sylph_preprocess_u8 writes for a host-made copy of the
 * view.  Crop-then-resize: a pixel outside the crop never contributes (this is not Pillow's resize(box=...)).  Several views may name
 * the same source pointer: the source is uploaded once, whatever the number of views.  All arrays are host arrays of B entries.  A crop
 * that leaves its source, or a non-positive size, fails with a message and launches nothing.  Makes the padded batch current. */
int sylph_preprocess_views(sylph_ctx* ctx, int B, const unsigned char* const* src_dev, const int* src_h, const int* src_w,
                           const int* crop_x0, const int* crop_y0, const int* crop_w, const int* crop_h, const int* new_h, const int* new_w,
                           const int* flip, int rgb_input, int* padded_h, int* padded_w);
/* Boundary/test entry: the normalised, padded network input of the current batch as (B,3,H,W) fp32 NCHW. */
int sylph_export_input(sylph_ctx* ctx, float* out_nchw_dev);

/* self.backbone(images.tensor) (meta_one_stage_detector.py:181,273): ResNet-FPN on the current batch. */
int sylph_backbone_fpn(sylph_ctx* ctx);

/* Boundary/test entry: make (B, padded H, W) the current batch and load its FPN pyramid from
 * nlevels device tensors (B,256,h_l,w_l) fp32 NCHW.  heights/widths: per-image unpadded sizes. */
int sylph_import_pyramid(sylph_ctx* ctx, int B, int padded_h, int padded_w, const int* heights, const int* widths,
                         const float* const* levels_nchw_dev);
/* Copy level `level` of the current pyramid to a (B,256,h_l,w_l) fp32 NCHW device tensor. */
int sylph_export_pyramid(sylph_ctx* ctx, int level, float* out_nchw_dev);

/* MetaFCOSHead.forward with support_set_per_class_code (sylph/modeling/meta_fcos/fcos.py:582-667;
 * CondConvBasic sylph/modeling/meta_fcos/head_utils.py:60-81).  cls_conv_dev: (N,256,k,k) fp32 with k = cg_code_ksize
 * (1: (N,256); 3: a 3x3 cross-correlation with zero padding 1 of the NORMALISED tower output), cls_bias_dev: (N) fp32 or NULL.
 * Results stay in the context (see sylph_export_head). */
int sylph_fcos_head(sylph_ctx* ctx, const float* cls_conv_dev, const float* cls_bias_dev, int N);
/* The same for a batch whose images belong to DIFFERENT episodes: image i is run with the codes of episode image_episode[i], and its head
 * outputs (and the detections sylph_decode_nms then returns for it) are those of sylph_fcos_head with that episode's codes on the same
 * batch -- bit for bit in bf16.  Everything in front of the class-conditional conv is class-agnostic (fcos.py:582-667,
 * head_utils.py:60-81), so one large step can serve the queries of many episodes; it stands for that many turns of the reference's
 * batch-1 query loop (sylph/evaluation/meta_learn_evaluation.py:421-426).
 * cls_conv_dev: (sum_e N_e, 256) fp32, episode after episode; cls_bias_dev: (sum_e N_e) fp32 or NULL; n_classes: host, E entries,
 * each >= 1; image_episode: host, B entries in [0, E).  An episode that no image uses is allowed.
 * Afterwards sylph_decode_nms numbers classes within the image's own episode: classes_dev[i][k] < N_i, and the cand_dev ordinal is
 * (loc_base + loc) * N_i + cls.  sylph_export_head writes logits (B, max_e N_e, h, w); entries [i, n >= N_i] are unspecified.
 * bf16 with FCOS.NORM "GN" and every N_e <= 32 is one class-conditional launch for the whole batch; any other combination runs, per
 * episode, the kernel sylph_fcos_head picks for that N over the episode's images.
 * 1x1 codes only: with cg_code_ksize 3 (CLS_LAYER kernel size 3) the call fails. */
int sylph_fcos_head_episodes(sylph_ctx* ctx, int E, const float* cls_conv_dev, const float* cls_bias_dev, const int* n_classes,
                             const int* image_episode);
/* The dual case: EVERY image of the batch is scored against G code sets in one step.  The result for (image i, set g) -- head outputs,
 * and the detections sylph_decode_nms_codesets then returns for it -- is that of sylph_fcos_head with set g's codes on the same batch, bit
 * for bit.  Only the class-conditional conv reads the codes (fcos.py:582-667, head_utils.py:60-81): the towers, the box / centerness / IoU
 * heads and the cls GroupNorm statistics run ONCE per call, not once per set.  It stands for the G query passes of the reference's
 * TEST.REPEAT_TEST protocol, one per support seed over the same query set (sylph/runner/meta_fcos_runner.py:451-672, each pass the batch-1
 * loop of sylph/evaluation/meta_learn_evaluation.py:421-426), or for one served frame scored for G tenants' class sets.
 * cls_conv_dev: (sum_g N_g, 256) fp32, set after set; cls_bias_dev: (sum_g N_g) fp32 or NULL; n_classes: host, G entries, each >= 1.
 * bf16 with FCOS.NORM "GN": the sets of up to 32 classes share one streaming pass over the tower output per 128 packed classes; any
 * other set runs the kernel sylph_fcos_head picks for its N, on the tower output normalised once.
 * sylph_export_head then writes logits (B, sum_g N_g, h, w), set after set.  The detections come from sylph_decode_nms_codesets;
 * sylph_decode_nms fails after this call.  1x1 codes only: with cg_code_ksize 3 (CLS_LAYER kernel size 3) the call fails. */
int sylph_fcos_head_codesets(sylph_ctx* ctx, int G, const float* cls_conv_dev, const float* cls_bias_dev, const int* n_classes);
/* MetaFCOSHead.forward with support_set_per_class_code = None -> forward_base_train (fcos.py:543-578): the towers and the checkpoint's
 * OWN classifier `cls_logits` (nn.Conv2d(256, NUM_CLASSES, CLS_LOGITS_KERNEL_SIZE 1 or 3, padding k // 2), fcos.py:418-427) -- the base
 * detector (run_type None) and evaluation with the pretrained codes.  *num_classes receives NUM_CLASSES. */
int sylph_fcos_head_pretrained(sylph_ctx* ctx, int* num_classes);
/* logits (B,N,h,w), reg (B,4,h,w) = relu(scale_l*bbox_pred), ctr (B,1,h,w), iou (B,1,h,w); NULL skips. */
int sylph_export_head(sylph_ctx* ctx, int level, float* logits_nchw_dev, float* reg_nchw_dev, float* ctr_nchw_dev,
                      float* iou_nchw_dev);

/* Boundary/test entry, inverse of sylph_export_head: load level `level` of the head outputs of the current batch from
 * fp32 NCHW device tensors (logits (B,N,h,w), reg (B,4,h,w) already relu(scale*bbox_pred), ctr (B,1,h,w), iou (B,1,h,w);
 * NULL leaves that plane untouched), so that sylph_decode_nms can be driven with known head outputs (the
 * predict_proposals / ml_nms / detector_postprocess known-answer cases, fcos_outputs.py:904-1028). */
int sylph_import_head(sylph_ctx* ctx, int N, int level, const float* logits_nchw_dev, const float* reg_nchw_dev,
                      const float* ctr_nchw_dev, const float* iou_nchw_dev);

/* FCOSOutputs.predict_proposals + select_over_all_levels + detector_postprocess
 * (sylph/modeling/meta_fcos/fcos_outputs.py:743-812,904-1028; meta_one_stage_detector.py:288-296).
 * out_heights/out_widths (host, may be NULL = image size): the "height"/"width" of each input dict.
 * Device outputs, row-major [B][max_out][...]; counts_dev[B]; status_dev[1] (bit0 candidate
 * overflow, bit1 output truncated).  cand_dev: (level, location, class) ordinal of each detection.
 * Decode reads the outputs of the most recent head call (sylph_fcos_head, sylph_fcos_head_episodes, sylph_fcos_head_pretrained or sylph_import_head) of the
 * current batch; any order of stage calls on one context is valid (a head need not be followed by a decode, a decode may be repeated,
 * and a decode that reported a status bit leaves nothing behind for the next one).  After sylph_fcos_head_codesets the call fails:
 * that head's G * B results go through sylph_decode_nms_codesets. */
int sylph_decode_nms(sylph_ctx* ctx, const int* out_heights, const int* out_widths, int max_out, float* boxes_dev,
                     float* scores_dev, int* classes_dev, int* levels_dev, float* locations_dev, int* cand_dev,
                     int* counts_dev, int* status_dev);
/* The decode of a sylph_fcos_head_codesets call: predict_proposals + select_over_all_levels + detector_postprocess
 * (fcos_outputs.py:743-812,904-1028; meta_one_stage_detector.py:288-296) once per (set, image), as the G query passes of
 * meta_fcos_runner.py:451-672 run them.  The threshold, PRE_NMS_TOPK per (image, level), the per-class NMS and POST_NMS_TOPK per image act
 * inside one set; classes are numbered within their own set (classes_dev < N_g) and the cand_dev ordinal is (loc_base + loc) * N_g + cls.
 * Device outputs as for sylph_decode_nms, row-major [G][B][max_out][...]; counts_dev[G * B]; ONE status_dev.  G must equal the last
 * head call's; after any other head entry the call fails (use sylph_decode_nms), as sylph_decode_nms fails after a code-sets head: a
 * caller's B-sized buffers are never overrun.  The ordering rules of sylph_decode_nms hold: the decode may be repeated, the head need not
 * be decoded, and a decode that reported a status bit leaves nothing behind for the next one. */
int sylph_decode_nms_codesets(sylph_ctx* ctx, int G, const int* out_heights, const int* out_widths, int max_out, float* boxes_dev,
                              float* scores_dev, int* classes_dev, int* levels_dev, float* locations_dev, int* cand_dev,
                              int* counts_dev, int* status_dev);

/* Query records: score new class codes on stored tower outputs.
 * Everything MetaFCOSHead.forward computes in front of the class-conditional conv is class-agnostic (fcos.py:582-667: the towers, bbox_pred,
 * ctrness, iou_overlap; the codes enter in CondConvBasic alone).  The reference's evaluation runs the same query set once per support seed and
 * per shot setting (meta_learn_evaluation.py:367-470 per pass, meta_fcos_runner.py:451-672 over TEST.REPEAT_TEST and the shot settings) and
 * pays the whole network every time.  A record keeps what one pass left, so that codes which arrive later are scored without the backbone and
 * the towers: any head entry followed by its decode on a loaded record gives, bit for bit, what it gives on the fresh batch.
 *
 * sylph_fcos_towers: the class-agnostic part of MetaFCOSHead.forward (fcos.py:582-667 up to the cls_logits call) on the current fresh
 * batch, with no class codes.  It leaves no logits: a decode or a head export after it fails as before any head call. */
typedef struct sylph_record sylph_record;
int sylph_fcos_towers(sylph_ctx* ctx);
/* Snapshot of what the towers left for the current fresh batch: the cls tower output, where its last GroupNorm is deferred (bf16 with
 * FCOS.NORM "GN") un-normalised together with that GroupNorm's coefficient and partial-statistics tables, otherwise normalised; the box /
 * centerness / IoU predictions; B, the padded H and W and the per-image sizes.  Valid after sylph_fcos_towers or after any head entry of
 * the batch -- except one that has applied the deferred GroupNorm in place (a bf16 head of more than 32 classes with the fused scan
 * switched off, the pretrained head, a logits export after a fused scan): the call then fails and names the remedy, sylph_fcos_towers
 * again.  The record is immutable, owned by the caller, allocated by the context (counted in sylph_device_bytes) and independent of the
 * plan cache.  On an allocation failure the error names the bytes asked for and nothing stays allocated. */
int sylph_record_store(sylph_ctx* ctx, sylph_record** out);
/* Make the record the current batch (the query loop of meta_learn_evaluation.py:421-426 from its stored tower outputs).  sylph_fcos_head,
 * sylph_fcos_head_episodes, sylph_fcos_head_codesets, sylph_fcos_head_pretrained, sylph_decode_nms, sylph_decode_nms_codesets and
 * sylph_export_head then work as on the fresh batch but launch no tower: the bf16 streaming kernels (up to 32 classes, the code-sets and
 * mixed-episode kernels, the fused scan) read the record in place; the other routes copy it into the plan's buffers first.
 * sylph_preprocess*, sylph_import_pyramid and sylph_import_head make a fresh batch current again.  The entries that need the pyramid
 * (sylph_backbone_fpn, sylph_export_pyramid, sylph_codegen*, sylph_roi_align*, the backbone and tower taps) and sylph_fcos_towers fail and
 * name the record.  A record made under another dtype, or under a sylph_config with another tower norm, level count, strides or code kernel size, is refused. */
int sylph_record_load(sylph_ctx* ctx, const sylph_record* rec);

/* Fine-tuning the class-conditional layer on the current batch's stored tower outputs: the classifier half of the TFA protocol the
 * reference compares against (MODEL.TFA.*, FREEZE_CLS_TOWER, FREEZE_BBOX_TOWER), where the last classifier layer -- CondConvBasic's
 * codes, or the base detector's cls_logits -- is trained on the K shots.  configs/COCO-Detection/TFA/FCOS_finetune.yaml and the
 * "-simplified" yamls train the classifier only (FREEZE_BBOX_BRANCH); the Meta-FCOS-pretrain-tfa-finetune yamls of each dataset also train
 * the box branch: sylph_box_samples / sylph_box_grad / sylph_set_box_branch below.  The three entries act on the current batch, a fresh one after sylph_fcos_towers (or
 * a head entry) or a loaded query record, bf16 with the deferred last GroupNorm and 1x1 codes; fp32 / f32s contexts, FCOS.NORM "none",
 * 3x3 codes and the ROIEncoder are refused by name.  None of them changes anything a later sylph_fcos_head* / sylph_decode_nms* on the
 * same batch or record reads.
 *
 * sylph_fcos_targets: FCOSOutputs.compute_targets_for_locations + get_sample_region (fcos_outputs.py:193-349), labels only.  n_gt boxes
 * (x0, y0, x1, y1) in network-input pixels with their class index and image index, sorted by image, all device arrays; sizes_of_interest:
 * host, nlevels - 1 values (MODEL.FCOS.SIZES_OF_INTEREST); center_sample / pos_radius: MODEL.FCOS.CENTER_SAMPLE / POS_RADIUS.
 * labels_out_dev: one int32 per row of the tower output (B * rows-per-image, the row order of the logits): the class index of the
 * smallest-area box that claims the location (the lowest index among equal areas), -1 for background; every location of the padded map
 * gets a label, as in the reference.  num_pos_out_dev: one int32, the number of rows with a label >= 0 (fcos_outputs.py:646). */
int sylph_fcos_targets(sylph_ctx* ctx, int n_gt, const float* boxes_dev, const int* gt_class_dev, const int* gt_image_dev,
                       const float* sizes_of_interest, int n_soi, int center_sample, float pos_radius, int* labels_out_dev,
                       int* num_pos_out_dev);
/* Bytes of workspace sylph_cls_grad needs for the current batch (the per-unit partial sums of one class block; N does not change it). */
int sylph_cls_grad_bytes(sylph_ctx* ctx, int N, int64_t* bytes_out);
/* Loss and gradient of the classification loss of FCOSOutputs.fcos_losses (fcos_outputs.py:640-660: sigmoid_focal_loss_jit(logits, one-hot,
 * alpha, gamma, reduction "sum"), NOT yet divided by num_pos_avg -- the caller normalises) with respect to the class codes, through
 * CondConvBasic (head_utils.py:60-81): logits = cls_tower . bf16(cls_conv)^T + cls_bias on the operand values sylph_fcos_head serves.
 * cls_conv_dev (N, 256) fp32 and cls_bias_dev (N) fp32 or NULL: device; class n of this call is label class_offset + n, so that a large
 * class set may be passed in pieces (the loss is separable per class).  Any N: one pass over the tower output per 32 classes.
 * loss_out_dev: one float, the sum over rows and the N classes; grad_w_out_dev (N, 256), grad_b_out_dev (N) or NULL.  The same inputs
 * give the same bits on every call. */
int sylph_cls_grad(sylph_ctx* ctx, const int* labels_dev, const float* cls_conv_dev, const float* cls_bias_dev, int N, int class_offset,
                   float alpha, float gamma, void* workspace_dev, float* loss_out_dev, float* grad_w_out_dev, float* grad_b_out_dev);
/* Fine-tuning the box branch -- bbox_pred (4) + ctrness (1) + iou_overlap (1), one 3x3 conv on the frozen bbox tower, and the per-level
 * Scales -- on the K shots: what _freeze_detector_head (meta_one_stage_detector.py:141-155) leaves trainable under the
 * Meta-FCOS-pretrain-tfa-finetune yamls (FREEZE_BBOX_TOWER on, FREEZE_BBOX_BRANCH off), trained by loss_fcos_loc / loss_fcos_ctr /
 * loss_fcos_iou (fcos_outputs.py:86-91, 675-741).  bf16 with FCOS.NORM "GN" / "NaiveGN" (the bbox tower's last GroupNorm is deferred);
 * fp32 / f32s contexts, FCOS.NORM "none" and the ROIEncoder are refused by name.  LOC_LOSS_TYPE is "giou".
 *
 * sylph_box_samples: the box-sample bank of the current FRESH batch (after sylph_fcos_towers or a head entry; a loaded record is refused by
 * name: it holds no bbox tower).  The first nine arguments and the assignment rule are sylph_fcos_targets'.  For every positive location,
 * in ascending row order (the order does not depend on the grid: a scan, no atomics), sample p is
 *   info_out_dev[p]     int32 (row, level, index of the claiming box, its class)
 *   targets_out_dev[p]  fp32 (l, t, r, b) / stride, plain fp32 as compute_targets_for_locations + fcos_outputs.py:185-189
 *   patches_out_dev[p]  bf16 [3][3][256]: bf16(relu(fma(x, a, b))) of the bbox tower's last layer at the nine neighbours (ky, kx), from the
 *                       deferred GroupNorm's coefficient table -- the operand values of the served prediction conv; zeros outside the map
 * count_out_dev[0] is the number of positives, also when it exceeds max_samples; then status_dev[0] = 1 (else 0) and nothing is written
 * past the capacity.  Nothing a later head / decode on the batch reads is changed. */
int sylph_box_samples(sylph_ctx* ctx, int n_gt, const float* boxes_dev, const int* gt_class_dev, const int* gt_image_dev,
                      const float* sizes_of_interest, int n_soi, int center_sample, float pos_radius, int max_samples, void* patches_out_dev,
                      float* targets_out_dev, int* info_out_dev, int* count_out_dev, int* status_dev);
/* Bytes of workspace sylph_box_grad needs for a bank of n samples (0 for n = 0). */
int sylph_box_grad_bytes(sylph_ctx* ctx, int n, int64_t* bytes_out);
/* Loss and gradient of the box losses of FCOSOutputs.fcos_losses (fcos_outputs.py:675-741) over a bank of n samples, with respect to the
 * box branch: w_dev (Cout, 256, 3, 3) fp32 in torch order, b_dev (Cout), scales_dev (levels), all device.  Needs no current batch.
 *   z = patch . bf16(w)^T + b (fp32 accumulation); reg = relu(scale_level z[0:4]); ious, gious: iou_loss.py:26-65; centerness targets:
 *   fcos_outputs.py:52-60; quality: 1 = BOX_QUALITY ["ctrness"], 2 = ["iou"], 3 = both; iou_mask: MODEL.FCOS.IOU_MASK (IoU targets
 *   below 0.3 become 0).  All targets are constants; the gradient passes the ReLU (zero where scale z <= 0) and reaches the scales.
 * sums_out_dev[4], UN-normalised: sum weight (1 - giou) (weight = the centerness target with "ctrness", else 1), the centerness BCE sum,
 * the IoU-quality BCE sum, sum of the centerness targets: the caller divides as fcos_outputs.py:698-738 (loc by max(sums[3], 1e-6) or by
 * num_pos, the other two by num_pos).  Channel 4 receives a gradient only with "ctrness", channel 5 only with "iou" (the reference
 * detaches the other loss).  grad_w_out_dev (Cout, 256, 3, 3), grad_b_out_dev (Cout), grad_scales_out_dev (levels): of the un-normalised
 * sum of the losses that are on.  z_out_dev / g_out_dev: NULL, or (n, Cout) pre-activations / d loss / d z.  n = 0 gives zeros.
 * No atomics: fixed units of 32 samples summed in a fixed order, the same bits on every call and grid. */
int sylph_box_grad(sylph_ctx* ctx, int n, const void* patches_dev, const float* targets_dev, const int* info_dev, const float* w_dev,
                   const float* b_dev, const float* scales_dev, int quality, int iou_mask, void* workspace_dev, float* sums_out_dev,
                   float* grad_w_out_dev, float* grad_b_out_dev, float* grad_scales_out_dev, float* z_out_dev, float* g_out_dev);
/* The box branch the context runs: Cout (5 or 6), the level count and the branch stamp (0: the finalized tensors); NULL skips. */
int sylph_box_branch_shape(sylph_ctx* ctx, int* cout, int* nlevels, uint64_t* stamp);
/* Host copies of the box branch: w_host (Cout, 256, 3, 3) bbox_pred | ctrness | iou_overlap stacked, b_host (Cout), scales_host (levels). */
int sylph_get_box_branch(sylph_ctx* ctx, float* w_host, float* b_host, float* scales_host);
/* Install another box branch: the prediction conv's packed weights, its tap table, biases and the level scales are re-packed as
 * sylph_finalize_weights packs them, and every cached plan is dropped (their segment tables carry the old scales): no batch is current
 * afterwards, and from the next batch on every tower / head step is bit-identical to a context finalized with these tensors.  Three NULLs
 * restore the finalized tensors.  The context carries a branch stamp: 0 for the finalized tensors, a fresh value per set, 0 again after a
 * restore; a query record keeps the stamp it was stored under and sylph_record_load refuses a record with another stamp, naming the
 * remedy (its stored predictions come from another branch). */
int sylph_set_box_branch(sylph_ctx* ctx, const float* w_host, const float* b_host, const float* scales_host);

/* Meta-training of the code generator on a frozen detector: the second stage of the paper, the recipes
 * configs/LVISv1-Detection/Meta-FCOS/Meta-FCOS-finetune-{once,2,sylph-fa}.yaml and configs/COCO-Detection/Meta-FCOS/Meta-FCOS-finetune-lvis.yaml
 * (BACKBONE.FREEZE, FREEZE_CLS_TOWER, FREEZE_BBOX_BRANCH on, CODE_GENERATOR.FREEZE off).  With a frozen backbone the 7x7x256 ROI maps of
 * the support instances are constants (sylph_roi_rows), with frozen towers the query side of an episode is a query record, and
 * sylph_cls_grad gives d loss / d (code, bias); the entries below are the generator's training-mode forward and its backward.
 * bf16 contexts only.  Refused by name, before any launch: fp32 / f32s contexts, the ROIEncoder, 3x3 codes, WEIGHT_LAYER / SCALE_LAYER
 * heads, BIAS_L2_NORM, META_BIAS, a TOWER_LAYERS entry other than ["GN", "ReLU"], idx out of range, seg_len that does not sum to M. */
/* The ROIPooler call of sylph_roi_align_rois (code_generator.py:341-348,928-930) written straight to the caller's (R, 49, 256) bf16
 * position-major device buffer: one launch, no per-ROI export, no temporary allocation; the values are exactly those of
 * sylph_roi_align_rois.  boxes_dev (R, 4) device, roi_image (R) host.  This is the ROI bank: it depends on the backbone only. */
int sylph_roi_rows(sylph_ctx* ctx, int R, const float* boxes_dev, const int* roi_image, void* rows_out_dev);
/* The generator's trainable tensors under the context's config as (state-dict key, offset, element count) triples in ONE flat fp32
 * vector: code_generator.code_generator_head.support_set_shared_tower.{3 i, 3 i + 1}.{weight, bias}, .support_set_cls_conv.0.*,
 * .support_set_cls_bias.0.* (BIAS_LAYER), .post_norm.* (POST_NORM "GN"), .conv_scale.scale (USE_WEIGHT_SCALE with POST_NORM or CONV_L2_NORM),
 * .bias_scale.scale (BIAS_LAYER) -- code_generator.py:341-402,648-688.  init_norm.* is never used by the forward and is not in the vector.
 * keys_out: max_entries x 128 bytes (NUL-terminated), or the three arrays NULL to ask for *n_out and *total_out (floats) alone. */
int sylph_codegen_param_layout(sylph_ctx* ctx, int max_entries, char* keys_out, int64_t* offset_out, int64_t* numel_out, int* n_out,
                               int64_t* total_out);
/* Host copy of the FINALIZED generator in that layout / install another one (NULL: restore the finalized one).  Install re-packs the
 * support convolutions, GroupNorm tables and tail constants as sylph_finalize_weights packs them, in place: cached support passes read the
 * new tensors from their next call on, and from then every sylph_codegen* / sylph_normalize_codes result is bit-identical to a context
 * finalized with those tensors.  Plans, the current batch and query records are not touched.  The context carries a generator stamp
 * (sylph_codegen_stamp): 0 for the finalized generator, a fresh value per set, 0 again after a restore; shot-bank rows are a function of
 * the generator, so a caller keeps the stamp with a bank (modelled on sylph_set_box_branch). */
int sylph_get_code_generator(sylph_ctx* ctx, float* flat_host);
int sylph_set_code_generator(sylph_ctx* ctx, const float* flat_host);
int sylph_codegen_stamp(sylph_ctx* ctx, uint64_t* stamp);
/* Workspace bytes of one training step on M shots in n_seg classes. */
int sylph_codegen_train_bytes(sylph_ctx* ctx, int M, int n_seg, int64_t* bytes_out);
/* What the binding and the tests need to know of a step's shape: the units of CGT_UNIT_SHOTS = 4 whole shots the weight gradient's row
 * reduction is cut into, its reduce passes (fan-in 8, the final one included), the floats of debug_out.  NULL skips. */
int sylph_codegen_train_shape(sylph_ctx* ctx, int M, int n_seg, int* units_out, int* passes_out, int64_t* debug_floats_out);
/* CodeGeneratorHead.forward_roi_align, training branch (code_generator.py:924-1002 with :766-875), on rows_dev (n_rows, 49, 256) bf16:
 * idx (host, M) selects bank rows, repeats allowed; the M shots are cut into n_seg consecutive segments of seg_len (host) shots.
 *   per tower layer i: y_i = conv3x3_pad1(x_i, bf16(W_i)) + b_i; x_{i+1} = bf16(relu(GroupNorm32(y_i)))  (statistics per shot, fp32, eps 1e-5)
 *   c[s] = mean_49(conv3x3_pad1(x_L, bf16(W_cls))) + b_cls, computed as Xsum[s] . bf16(W_cls)^T / 49 with Xsum the box sums of x_L (the
 *   pool commutes with the conv); rb[s] likewise (0 without BIAS_LAYER); code_raw[j], bias_raw[j] = the shot means of segment j
 *   code[j] = conv_scale * l2_normalize(GroupNorm32(code_raw[j]));  bias[j] = bias_scale * bias_raw[j] - log((1 - PRIOR_PROB) / PRIOR_PROB)
 * params_dev: the caller's fp32 master copy in the layout above.  codes_out_dev (n_seg, 257): code ++ bias, what sylph_fcos_head and
 * sylph_cls_grad take.  Saved activations stay in workspace_dev (sylph_codegen_train_bytes).  Needs no current batch. */
int sylph_codegen_train_forward(sylph_ctx* ctx, const float* params_dev, const void* rows_dev, int n_rows, int M, const int* idx, int n_seg,
                                const int* seg_len, void* workspace_dev, float* codes_out_dev);
/* The backward of the preceding forward (the same workspace, params, rows, n_rows, M, n_seg): grad_codes_dev (n_seg, 257) =
 * d loss / d codes_out -> grad_out_dev, flat in the layout above; a tensor that receives no gradient holds exact zeros.  Every rounding of
 * the forward is treated as the identity; d y_i is rounded to bf16 where it enters the data- and weight-gradient MFMAs, all else is fp32.
 * No atomics: the weight gradient's rows are summed per unit and the units in a fixed order, the same bits on every call and on every grid
 * (SYLPH_CODEGEN_TRAIN_BLOCKS caps the blocks).  debug_out_dev: NULL, or sylph_codegen_train_shape's floats: every stage in fp32 --
 *   per layer i: y_i (M 49, 256) | (mean, rstd) (M, 32, 2) | x_{i+1} as stored; Xsum (M, 2304) | c (M, 256) | rb (M) | code_raw (n_seg, 256) |
 *   bias_raw (n_seg) | d code_raw | d bias_raw | d c (M, 256) | d rb (M) | with a tower: d Xsum (M, 2304) | d x_L | for i = L - 1 .. 0:
 *   d y_i | d x_i (i >= 1). */
int sylph_codegen_train_backward(sylph_ctx* ctx, const float* params_dev, const void* rows_dev, int n_rows, int M, int n_seg,
                                 void* workspace_dev, const float* grad_codes_dev, float* grad_out_dev, float* debug_out_dev);
/* Batch size, padded size and device bytes of a record; NULL skips. */
int sylph_record_info(const sylph_record* rec, int* B, int* padded_h, int* padded_w, int64_t* bytes);
/* Release a record, with the context that stored it (the stream is drained first).  If it is the current batch, no batch is current
 * afterwards.  sylph_ctx_destroy releases the records that are still alive. */
void sylph_record_destroy(sylph_ctx* ctx, sylph_record* rec);

/* Merge of the detections of several views of the same source (sylph_preprocess_views): one class-wise NMS over their union, in the
 * coordinates of the source.  The per-view decode is sylph_decode_nms with out_heights / out_widths = the view's CROP size: its boxes are
 * in crop pixels, clipped to the crop, in the mirrored crop for a flipped view.  Decode writes [B][max_out] rows, so the views of several
 * steps land in consecutive slices of one [n_views][max_in] buffer set (boxes_dev [.][4], scores_dev, classes_dev; counts_dev[n_views]).
 * Host arrays of n_views entries: view_src (in [0, n_src)), view_x0 / view_y0 (crop origin), view_w (crop width), view_flip.  Per source:
 *   1  back to source coordinates: flipped (x1, x2) <- (w - x2, w - x1); then x += x0, y += y0; plain fp32 in that order, no clip
 *   2  pool: the rows of its views in ascending view index, rows in order (the views of a source need not be adjacent)
 *   3  stable sort by score, descending: a tie goes to the lower view index, then to the lower row
 *   4  greedy class-aware NMS with MODEL.FCOS.NMS_TH: inter / (area_i + area_j - inter) > thr suppresses, equal classes only; thr <= 0: off
 *   5  keep: the first POST_NMS_TOPK_TEST kept boxes and every later kept box whose score equals the K-th; K <= 0 keeps all
 * Outputs, row-major [n_src][max_out]: boxes, scores, classes, and out_view_dev / out_row_dev: the input row each output came from;
 * out_counts_dev[n_src]; status_dev[1]: bit1 (value 2) = a source was truncated at max_out.  A source whose views could hold more than
 * MERGE_POOL_CAP = 4096 rows together (max_in x its views) fails by name before any launch.  Needs no current batch; nothing is kept
 * between calls.  The rows are taken as decode left them, clipped to the crop: rows that a crop border cut can overlap more than they did
 * under the view's own NMS, and the fragments of one object that several tiles cut share too little to suppress each other:
 * sylph_stitch_views (below) joins them. */
int sylph_merge_views(sylph_ctx* ctx, int n_src, int n_views, const int* view_src, const float* view_x0, const float* view_y0,
                      const float* view_w, const int* view_flip, int max_in, const float* boxes_dev, const float* scores_dev,
                      const int* classes_dev, const int* counts_dev, int max_out, float* out_boxes_dev, float* out_scores_dev,
                      int* out_classes_dev, int* out_view_dev, int* out_row_dev, int* out_counts_dev, int* status_dev);
/* The same merge for sources of any size: inputs, outputs and the rules 1 - 5 are those written above sylph_merge_views, and on every
 * input that both entries accept the result is the same bit for bit.  The pool lives in the caller's workspace_dev (16-byte aligned, any
 * contents, nothing is kept in it between calls) of at least sylph_merge_views_large_bytes(n_src, n_views, max_in) bytes: about 33 bytes
 * per row of the [n_views][max_in] buffers rounded up to a power of two; the function returns -1 and sets sylph_last_error() for a
 * non-positive argument or n_views * max_in >= 2^31.  topk is rule 5's K: above 0 that many, 0 keeps every kept box, -1 takes
 * POST_NMS_TOPK_TEST.  A source whose views could hold more than MERGE_LARGE_POOL_CAP = 1048576 rows together (max_in x its views), a NULL
 * workspace and a workspace smaller than the bytes function says fail by name before any launch.  status_dev[0] is cleared by the call;
 * bit1 (value 2) = a source was truncated at max_out, whose first max_out rows in order are then written.  The call runs on the context's
 * stream and reads nothing back; like sylph_merge_views its only wait is for the previous merge call's upload of the view tables to have
 * left the host copy, never for a kernel.  It needs no current batch and works while a query record is loaded.
 * Class ids are any int32, compared for equality only; a count outside [0, max_in] is clamped. */
int64_t sylph_merge_views_large_bytes(int n_src, int n_views, int max_in);
int sylph_merge_views_large(sylph_ctx* ctx, int n_src, int n_views, const int* view_src, const float* view_x0, const float* view_y0,
                            const float* view_w, const int* view_flip, int max_in, const float* boxes_dev, const float* scores_dev,
                            const int* classes_dev, const int* counts_dev, int topk, int max_out, float* out_boxes_dev,
                            float* out_scores_dev, int* out_classes_dev, int* out_view_dev, int* out_row_dev, int* out_counts_dev,
                            int* status_dev, void* workspace_dev, int64_t workspace_bytes);

/* The merge that stitches what tile borders cut: an object that a crop border cuts comes back as a clipped fragment from every tile that
 * sees part of it, and rule 4 keeps them all.  Inputs and outputs are those of sylph_merge_views_large plus the host arrays view_h
 * [n_views] (crop heights), src_w / src_h [n_src] (source sizes), stitch_thr in (0, 1], border_px >= 0 and one more output,
 * out_stitched_dev [n_src][max_out] int32.  Rules 1, 2, 3 and 5 are those written above sylph_merge_views; plain fp32 in the order written:
 *   0  the cut flag of a row, after rule 1, box (x1, y1, x2, y2) in source pixels, crop L = x0, T = y0, R = x0 + w, B = y0 + h: cut iff
 *      (L > 0 and x1 <= L + border_px) or (R < src_w and x2 >= R - border_px) or (T > 0 and y1 <= T + border_px) or
 *      (B < src_h and y2 >= B - border_px).  A crop border that is the source's own never cuts: a full-frame view has no cut row
 *   M  the pair test, equal classes, i before j in rule-3 order, inter as in rule 4, areas (x2 - x1) * (y2 - y1): if i or j is cut,
 *      inter / fminf(area_i, area_j) > stitch_thr (intersection over the smaller box; 0 / 0 is NaN: false); otherwise rule 4's test
 *      with NMS_TH, and NMS_TH <= 0 means that such pairs never match
 *   4a walk the rows in rule-3 order: row j is kept unless an earlier kept row matches it; its keeper is the FIRST kept row i, in keep
 *      order, with M(i, j); matching always uses the keeper's ORIGINAL box.  Every kept row i carries a union box U_i, at first its own
 *      box; a cut pair grows it, U_i <- the component-wise hull (fminf / fmaxf) of U_i and box j, and adds 1 to stitched_i; an uncut
 *      pair only suppresses
 *   4b drop only, nothing grows: walk the kept rows in order; a kept row k that is cut is dropped if an earlier surviving row i of its
 *      class has inter(U_i, box_k) / area(box_k) > stitch_thr, U_i as 4a left it; the first such i gets stitched_i += 1; what k had
 *      absorbed itself is not passed on
 *   5  on the survivors with their own scores.  An output row carries U as its box, the survivor's score, class, view and row, and
 *      out_stitched = 1 + its count
 * With no cut row in the pool every output equals sylph_merge_views_large's bit for bit and out_stitched is 1 everywhere.  The hull does
 * not depend on an order, so the bits are reproducible.  Fragments match on their original boxes: two fragments that no row bridges
 * are joined only while the object is narrower than about 3 x the overlap strip (at stitch_thr 0.5); larger objects rely on a full-frame
 * view.  workspace_dev: at least sylph_stitch_views_bytes(n_src, n_views, max_in) bytes, never fewer than the large merge's (about 77
 * bytes per row); -1 as sylph_merge_views_large_bytes.  Refused by name before any launch: stitch_thr outside (0, 1] or NaN, border_px
 * < 0 or NaN, a non-positive source or crop size, a crop that leaves its source, a NULL or short workspace, and what
 * sylph_merge_views_large refuses.  Stream, waits, status_dev, topk, class ids and counts: as sylph_merge_views_large. */
int64_t sylph_stitch_views_bytes(int n_src, int n_views, int max_in);
int sylph_stitch_views(sylph_ctx* ctx, int n_src, int n_views, const int* view_src, const float* view_x0, const float* view_y0,
                       const float* view_w, const float* view_h, const int* view_flip, const float* src_w, const float* src_h, int max_in,
                       const float* boxes_dev, const float* scores_dev, const int* classes_dev, const int* counts_dev, float stitch_thr,
                       float border_px, int topk, int max_out, float* out_boxes_dev, float* out_scores_dev, int* out_classes_dev,
                       int* out_view_dev, int* out_row_dev, int* out_stitched_dev, int* out_counts_dev, int* status_dev,
                       void* workspace_dev, int64_t workspace_bytes);

/* COCO bbox evaluation on detection rows, device side: what evaluator.evaluate() (sylph/evaluation/meta_learn_evaluation.py:465) hands to
 * pycocotools -- pycocotools/cocoeval.py evaluateImg (sylph_coco_match) and accumulate (sylph_coco_accumulate), useCats = 1 -- in float64, in the
 * operation order that tests/cocoeval_ref.py restates.  Pair p = image index * n_cat + category index, both in ascending id order.
 * sylph_coco_match: det_rows_dev (n_det, 8) fp32 rows (image id | x0 | y0 | x1 | y1 | score | class | valid) ALREADY ordered by (pair, score
 * descending, arrival); det_off_dev [n_pairs + 1] the rows of every pair.  Ground truth ordered by (pair, file order): gt_box_dev (G, 4) XYWH
 * f64, gt_area_dev (the annotation's area), gt_crowd_dev, gt_off_dev [n_pairs + 1]; max_gt = the most boxes any pair holds.  iou_thr_dev
 * [n_thr] and area_rng_dev [n_area][2] f64 as the host computed them.  Per pair the first max_det rows are matched greedily; per row
 * matched_dev / ignored_dev receive one bit per (area a, threshold t) at bit a * n_thr + t (later rows of a pair are left alone);
 * npig_dev [n_cat][n_area] is cleared and receives the non-ignored ground-truth count.  IoU = i / u with iw = min(dx + dw, gx + gw) - max(dx, gx),
 * 0 when iw or ih <= 0, u = crowd ? dw * dh : dw * dh + gw * gh - i.  A pair of up to sylph_coco_match_tile_gt(max_det) boxes keeps its IoU
 * tile on chip: SYLPH_COCO_MATCH_TILE_GT = 128 for max_det <= 131, fewer beyond (the tile is max_det x boxes float64 in 144 KiB of LDS: 55
 * boxes at max_det 300, 13 at 1024).  A larger pair recomputes the same expression per visit -- identical results -- and keeps its flags in
 * gt_scratch_dev: 64 bytes per ground-truth box (64 * G bytes for the G rows of gt_box_dev), any contents; it may be NULL only when
 * max_gt <= sylph_coco_match_tile_gt(max_det), and the call fails by name otherwise.  n_area <= 4, n_area * n_thr <= 40, max_det <= 1024.
 * n_det is the row count of det_rows_dev / matched_dev / ignored_dev; det_off_dev lives on the device and is not read by the host, so
 * det_off_dev[n_pairs] <= n_det and ascending offsets are the caller's contract (as gt_off_dev's are against gt_box_dev).
 * sylph_coco_accumulate: rows ordered by (category, score descending, image, rank) -- score_dev, rank_dev (rank inside the pair), the two masks --
 * with cat_off_dev [n_cat + 1]; per (category, area, maxDet) the tp / fp cumulative sums over rows of rank < maxDet, recall, the
 * right-to-left precision maximum and the rec_thr_dev [n_rec] look-ups (first index with recall >= threshold) ->
 * precision_dev [T][R][K][A][M], recall_dev [T][K][A][M], scores_dev [T][R][K][A][M] f64, -1 where npig = 0.  A category's segment is scanned in
 * chunks of SYLPH_COCO_ACC_CHUNK = 1024 rows and may be arbitrarily long.  n_thr <= 10, n_rec <= 128.  Neither call needs a current batch. */
#define SYLPH_COCO_MATCH_TILE_GT 128 /* ground-truth boxes of one pair whose IoU tile stays on chip, for max_det <= 131 */
#define SYLPH_COCO_ACC_CHUNK 1024    /* rows of a category's segment per scan step of sylph_coco_accumulate */
/* the bound that holds for this max_det (<= SYLPH_COCO_MATCH_TILE_GT; -1 for a max_det outside 1 .. 1024): no context, no device */
int sylph_coco_match_tile_gt(int max_det);
int sylph_coco_match(sylph_ctx* ctx, int n_det, const float* det_rows_dev, int n_pairs, int n_cat, const int* det_off_dev,
                     const double* gt_box_dev, const double* gt_area_dev, const int* gt_crowd_dev, const int* gt_off_dev, int max_gt, int n_thr,
                     const double* iou_thr_dev, int n_area, const double* area_rng_dev, int max_det, unsigned char* gt_scratch_dev,
                     unsigned long long* matched_dev, unsigned long long* ignored_dev, int* npig_dev);
int sylph_coco_accumulate(sylph_ctx* ctx, int n_det, const float* score_dev, const int* rank_dev, const unsigned long long* matched_dev,
                          const unsigned long long* ignored_dev, int n_cat, const int* cat_off_dev, const int* npig_dev, int n_thr, int n_rec,
                          const double* rec_thr_dev, int n_area, int n_maxdet, const int* max_dets_dev, double* precision_dev,
                          double* recall_dev, double* scores_dev);

/* LVIS (federated) bbox evaluation on detection rows, device side: what FewshotLVISEvaluator (sylph/evaluation/lvis_evaluation.py:246-250,
 * _evaluate_predictions_on_lvis_with_per_category: LVISResults + LVISEval.run()) hands to lvis-api -- lvis/eval.py evaluate_img (sylph_lvis_match)
 * and accumulate (sylph_coco_accumulate with n_maxdet = 1 and max_dets = [max_dets_per_image]: arithmetically the same) -- in float64, in
 * the operation order that tests/lviseval_ref.py restates.  The per-image budget (LVISResults.limit_dets_per_image), the federated filter
 * (LVISEval._prepare) and the pair list are the caller's (sylph_amd/lvis_eval.py, torch on the device).
 * sylph_lvis_match runs over a COMPACTED list of the (image, category) pairs that exist (detections or ground truth), never over a table
 * of images x categories.  max_pairs is a host-known upper bound of the pair count (it sizes the grid and the four per-pair arrays);
 * n_pairs_dev is the live count, one int on the device, which the host does not read: surplus waves return.  Per pair p < *n_pairs_dev:
 * pair_cat_dev[p] the category index (for npig), pair_flags_dev[p] bit 0 = the category is not exhaustively annotated in this image,
 * det_off_dev [max_pairs + 1] / gt_off_dev [max_pairs + 1] its rows of det_rows_dev (ordered by (pair, score descending, arrival); layout as
 * for sylph_coco_match) and of the ground truth (gt_box_dev (G, 4) XYWH f64, gt_area_dev, gt_ignore_dev, ordered by (pair, file order)).
 * A box is ignored in an area range when its ignore flag is set or its area is outside; detections walk the non-ignored boxes first, a
 * matched box is never matched again (no crowd boxes), and an unmatched detection is ignored when its own area w * h is outside the range or
 * the pair's flag bit 0 is set.  There is no cut inside a pair: a pair may hold up to max_det (= max_dets_per_image) detections,
 * max_det <= SYLPH_LVIS_MATCH_MAX_DETS = 1024; max_gt = the most boxes any pair holds.  matched_dev / ignored_dev / npig_dev as for
 * sylph_coco_match.  One wave per pair, four waves per block, each with an LDS slice of SYLPH_LVIS_MATCH_SLICE_BYTES = 36 KiB: a pair of D
 * detections and G boxes keeps its IoU tile and state rows there when 32 D + G (8 D + 64) <= 36864 -- sylph_lvis_match_fits(D, G), decided
 * per pair from its own counts: D = 300 fits 11 boxes, D = 64 fits 60, D = 1 fits 511 -- and otherwise recomputes the IoU per visit
 * (identical results) with its state rows in gt_scratch_dev: 64 bytes per ground-truth box, any contents; it may be NULL only when
 * sylph_lvis_match_fits(max_det, max_gt), and the call fails by name otherwise.  n_area <= 4, n_area * n_thr <= 40. */
#define SYLPH_LVIS_MATCH_SLICE_BYTES 36864 /* LDS of one wave = one pair: 32 B per detection, 8 B per IoU, 64 B per ground-truth box */
#define SYLPH_LVIS_MATCH_MAX_DETS 1024     /* detections of one pair, i.e. max_dets_per_image */
/* 1: a pair of n_det detections and n_gt boxes keeps its IoU tile on chip, 0: it needs the scratch; -1 for negative counts or
 * n_det > SYLPH_LVIS_MATCH_MAX_DETS.  No context, no device */
int sylph_lvis_match_fits(int n_det, int n_gt);
int sylph_lvis_match(sylph_ctx* ctx, int n_det, const float* det_rows_dev, int max_pairs, const int* n_pairs_dev, int n_cat,
                     const int* pair_cat_dev, const int* pair_flags_dev, const int* det_off_dev, const double* gt_box_dev,
                     const double* gt_area_dev, const int* gt_ignore_dev, const int* gt_off_dev, int max_gt, int n_thr,
                     const double* iou_thr_dev, int n_area, const double* area_rng_dev, int max_det, unsigned char* gt_scratch_dev,
                     unsigned long long* matched_dev, unsigned long long* ignored_dev, int* npig_dev);

/* CodeGenerator.forward / CodeGeneratorHead.forward_roi_align, eval branch
 * (sylph/modeling/code_generator/code_generator.py:924-1002): the current batch is the S support
 * images of ONE class; boxes_dev (S,4) fp32 XYXY (one gt box per image).  code_out_dev: 256 k^2 + 1 fp32 (k = cg_code_ksize;
 * 257 for the 1x1 codes) = un-normalised cls_conv[256 k^2] in (c, ky, kx) order ++ cls_bias[1].
 * With cg_type 1 this is ROIEncoder.forward (sylph/modeling/code_generator/roi_encoder.py:146-204,
 * S = EVAL_SHOT shots of one class): cls_conv[256] ++ cls_bias[1] (prior already added, no
 * normalisation step exists for this variant). */
int sylph_codegen(sylph_ctx* ctx, const float* boxes_dev, float* code_out_dev);
/* The same for SEVERAL classes in one batch (support-path throughput: C4 runs 866 classes x 5 shots through the R-101 backbone):
 * the current batch holds n_classes x shots support images, class k = images [k * shots, (k + 1) * shots); boxes_dev
 * (n_classes * shots, 4); codes_out_dev (n_classes, 256 k^2 + 1).  The reference computes one class per call
 * (meta_one_stage_detector.py:229-254); per class the arithmetic here is the same (ROIAlign, tower, GroupNorm and the shot mean
 * are per image / per class), only the launches are shared.  ROIEncoder (cg_type 1): shots = EVAL_SHOT; its encoder attends over
 * the class axis of a (classes, shots, C) tensor and sees one class per call at inference (roi_encoder.py:184-186), so a class of the
 * batch never meets another class's tokens here either: the codes are those of one call per class. */
int sylph_codegen_classes(sylph_ctx* ctx, const float* boxes_dev, int shots, float* codes_out_dev);
/* The same from a ROI LIST: R support instances over the current batch of B images, several per image if the image shows several.
 * ROI r is box boxes_dev[r] (XYXY, network-input coordinates) on image roi_image[r] in [0, B), in any order; an image may carry no
 * ROI or many.  The ROIs are cut into n_seg consecutive segments of seg_len[j] >= 1 ROIs (sum = R); row j of codes_out_dev
 * (n_seg, 256 k^2 + 1) is what ONE reference call of CodeGeneratorHead.forward_roi_align (code_generator.py:924-1002) or, with cg_type 1, of
 * ROIEncoder.forward (roi_encoder.py:146-204) gives for a support set of seg_len[j] shots whose shot i is the feature pyramid of the
 * segment's i-th ROI's image with that ROI's box.  The backbone has run once per image, not once per instance; segments never see
 * each other (shot softmax, compute_code, token mean and the length-1 attention stay inside a segment) and a segment may be longer
 * than 64 shots.  roi_image and seg_len are HOST arrays; their device copies are kept per (batch shape, R), shared with a
 * sylph_codegen[_classes] call where R = B, and uploaded again only when the values change.  Afterwards
 * sylph_codegen_weight_norm gives n_seg values and the support taps R rows (per-shot stages; SYLPH_SUP_CONTEXT stays per image:
 * B rows) or n_seg rows (class tokens). */
int sylph_codegen_rois(sylph_ctx* ctx, int R, const float* boxes_dev, const int* roi_image, int n_seg, const int* seg_len,
                       float* codes_out_dev);
/* Shot bank: the support path cut at its per-shot stage, so that the class codes of any draw of shots from a pool of instances cost
 * a gather and a combination, not a network pass (the reference runs CodeGeneratorHead.forward_roi_align / ROIEncoder.forward on the
 * support images of every seed and shot count again, meta_fcos_runner.py:497-560 over meta_learn_evaluation.py:256-365).
 * sylph_shot_row_floats: floats of one bank row under the context's config -- 256 k^2 + 4 (k = cg_code_ksize; 256 + 4 with cg_type 1). */
int sylph_shot_row_floats(sylph_ctx* ctx, int* n_out);
/* The support pass of sylph_codegen_rois up to the last stage that looks at one shot alone: rows_out_dev (R, row) fp32, row r for ROI
 * (roi_image[r], boxes_dev[r]) of the current batch.  CodeGenerator (code_generator.py:954-967 and utils.py:51-67, the per-shot half of
 * forward_roi_align :924-1002): [0, 256 k^2) the pooled cls_conv map in (c, ky, kx) order (global mean, or the (3, 3) adaptive
 * average), then the pooled bias term (BIAS_L2_NORM applied), the pooled shot-weight logit, the pooled class-scale term (0 for a head
 * the config lacks) and one 0 pad.  ROIEncoder (roi_encoder.py:146-186): the shot's token after the last encoder layer, four 0 pads.
 * The pass, its checks and its image table are those of sylph_codegen_rois (a call with the same list uploads no image table
 * again); fails on a loaded query record.  Rows are valid under the weights, dtype and generator config that made them. */
int sylph_codegen_shots(sylph_ctx* ctx, int R, const float* boxes_dev, const int* roi_image, float* rows_out_dev);
/* The class codes of segments drawn from a bank rows_dev (n_rows, row) of such rows: idx[M] (host, each in [0, n_rows), repeats
 * allowed) is cut into n_seg consecutive segments of seg_len[j] in [1, 16384] indices (host, sum = M); row j of codes_out_dev
 * (n_seg, 256 k^2 + 1) is, bit for bit, what sylph_codegen_rois gives for a segment holding those shots in that order: the shot
 * softmax or 1 / S and compute_code (code_generator.py:766-829), resp. the token mean and the two head FC stacks with the prior
 * (roi_encoder.py:184-204).  weight_norm_out_dev (may be NULL): n_seg cls_weight_norm values when the generator has a scale head
 * (code_generator.py:987-993), as sylph_normalize_codes takes them.  Needs no current batch and works on a loaded query record; every
 * failure names the offending position. */
int sylph_shot_combine(sylph_ctx* ctx, const float* rows_dev, int n_rows, int M, const int* idx, int n_seg, const int* seg_len,
                       float* codes_out_dev, float* weight_norm_out_dev);
/* How many sylph_codegen / sylph_codegen_classes / sylph_codegen_rois calls on this context had to upload their ROI tables (a repeated
 * list, or the same shots on the same batch shape, uploads none). */
int sylph_roi_table_uploads(sylph_ctx* ctx, int64_t* n_out);
/* With cg_has_scale: the "cls_weight_norm" outputs of the last sylph_codegen[_classes | _rois] call (one fp32 per class / segment), the factor
 * forward_normalize_code multiplies into the L2-normalised code (code_generator.py:838-840,987-993) -> pass them to
 * sylph_normalize_codes as weight_norm_dev. */
int sylph_codegen_weight_norm(sylph_ctx* ctx, float* weight_norm_out_dev);

/* Boundary/test entry: the ROIPooler call of the code generator alone (code_generator.py:341-348,928-930: box ->
 * level assignment -> ROIAlignV2 aligned, adaptive sampling, 7x7).  The current batch holds S images, boxes_dev (S,4)
 * one XYXY box per image; out_nchw_dev (S,256,7,7) fp32. */
int sylph_roi_align(sylph_ctx* ctx, const float* boxes_dev, float* out_nchw_dev);
/* The same ROIPooler call (code_generator.py:341-348,928-930) over a ROI list: R boxes, box r on image roi_image[r] (host array)
 * of the current batch; out_nchw_dev (R,256,7,7) fp32.  Row r equals sylph_roi_align's row on a batch whose image r is image
 * roi_image[r]; a box wholly outside its level gives zeros. */
int sylph_roi_align_rois(sylph_ctx* ctx, int R, const float* boxes_dev, const int* roi_image, float* out_nchw_dev);

/* CodeGeneratorHead.forward_normalize_code (code_generator.py:832-897): codes_dev (n, 256 k^2 + 1) in place, k = cg_code_ksize.
 * k = 3: GroupNorm(32, 256) on (1,256,3,3) -- a group is 8 channels x 9 taps -- then F.normalize(dim = 1) per tap over the channels.
 * weight_norm_dev: (n) cls_weight_norm factors applied after the L2 normalisation (code_generator.py:838-840), or NULL. */
int sylph_normalize_codes(sylph_ctx* ctx, float* codes_dev, int n, const float* weight_norm_dev);

/* reduce_class_code + replace ordering (sylph/modeling/code_generator/utils.py:376-427; the cross-rank step of the
 * base-class "use all ground truths" path, sylph/evaluation/meta_learn_evaluation.py:118-254): rows_dev (n, row_ld) packed
 * chunk codes = cls_conv[256] | cls_bias | acc_weight | class id | valid | cls_weight_norm | has_weight_norm | payload;
 * the rows of a class are summed in row order (acc_weight in double).  divide_by_acc != 0: the cross-rank reduce (sums
 * divided by the accumulated weight when |1 - acc| > 1e-6, acc_weight := 1); == 0: the per-rank accumulation of
 * len/total_len-weighted chunk codes (meta_learn_evaluation.py:176-188; acc_weight := accumulated weight).
 * out_dev (num_classes, row_ld): row c = class id c (valid = 0 when no chunk of that class exists).
 * The row layout fixes the code at 256 floats: with cg_code_ksize 3 (CLS_LAYER kernel size 3) the call fails. */
int sylph_reduce_codes(sylph_ctx* ctx, const float* rows_dev, int n, int row_ld, float* out_dev, int num_classes,
                       int divide_by_acc);

/* The episode's one collective through the C ABI (MetaFCOSRunner._gather_class_code, sylph/runner/meta_fcos_runner.py:381-439,
 * which pickles dicts through all_gather_object): local_dev (n_local, 280) packed class-code rows of this rank (row layout of
 * sylph_reduce_codes + 16 name lanes) -> out_dev (world * capacity, 280): every rank's block in rank order on every rank, unused
 * rows zero (valid = 0).  ONE in-place ncclAllGather of equal-size blocks on the context's stream (RCCL over xGMI); capacity is the
 * statically known shard size ceil(n_classes / world), so there is no count exchange and no host read-back.  comm: an ncclComm_t --
 * from sylph_comm_init_rank below or the host's own RCCL communicator.  librccl is resolved at first use (dlopen): the library has
 * no link-time dependency on it.  The Python host side keeps torch.distributed (backend "nccl" = RCCL) as its default.
 * Fails with cg_code_ksize 3 (CLS_LAYER kernel size 3), like sylph_reduce_codes. */
int sylph_allgather_codes(sylph_ctx* ctx, void* comm, const float* local_dev, int n_local, int capacity, float* out_dev);
/* Communicator helpers for hosts without their own RCCL binding: rank 0 makes the 128-byte id (ncclGetUniqueId), hands it to the
 * other ranks over any channel, every rank calls init_rank (ncclCommInitRank on the context's device). */
int sylph_comm_unique_id(char* id_out_128);
int sylph_comm_init_rank(sylph_ctx* ctx, const char* id_128, int nranks, int rank, void** comm_out);
int sylph_comm_destroy(void* comm);

/* Primitive entries used by the kernel parity tests (F.conv2d / F.group_norm equivalents).
 * x: (B,C,H,W) fp32 NCHW device; w_host: (Cout,Cin,KH,KW) fp32 host; scale/shift host (Cout) or NULL;
 * residual: (B,Cout,Ho,Wo) device or NULL; y: (B,Cout,Ho,Wo) fp32 device. */
int sylph_conv2d(sylph_ctx* ctx, const float* x_nchw_dev, int B, int C, int H, int W, const float* w_host, int Cout,
                 int KH, int KW, int stride, int pad, const float* scale_host, const float* shift_host, int relu,
                 const float* residual_nchw_dev, float* y_nchw_dev);
int sylph_group_norm(sylph_ctx* ctx, const float* x_nchw_dev, int B, int H, int W, const float* gamma_host,
                     const float* beta_host, int relu, float* y_nchw_dev);

/* Kernel parity test entry for the dedicated ResNet stem kernels (bf16 contexts only): x (B,3,H,W) fp32 NCHW device,
 * already normalised; w_host (64,3,7,7), scale/shift host (64) = folded FrozenBN.  stem_out (B,64,H/2,W/2) =
 * relu(bn(conv7x7 s2 p3)), pool_out (B,64,H/4,W/4) = maxpool 3x3 s2 p1 of it; either may be NULL.
 * (detectron2 BasicStem; call site meta_one_stage_detector.py:181,273.) */
int sylph_stem_maxpool(sylph_ctx* ctx, const float* x_nchw_dev, int B, int H, int W, const float* w_host,
                       const float* scale_host, const float* shift_host, float* stem_out_nchw_dev, float* pool_out_nchw_dev);

/* Parity taps (test boundary; no reference counterpart -- the reference's modules are called one by one from Python, so its
 * tests can look at any intermediate; these entries give the parity tests the same view of the fused HIP graph).
 * sylph_set_debug_taps(1) before the first head call of a batch shape: every FCOS tower layer keeps its stored conv output in
 * its own buffer (same kernels and launches, other destination) instead of the two ping-pong buffers.
 * sylph_export_stage: output of ResNet stage `stage` (2..5 = res2..res5) of the last sylph_backbone_fpn as
 * (B, C << (stage - 2), h, w) fp32 NCHW, C = 256 (64 for the BasicBlock depths 18 / 34) (detectron2 ResNet.forward outputs; call site meta_one_stage_detector.py:181,273).
 * MobileNetV2 (cfg.mobilenet): 24 / 32 / 96 / 320 channels at strides 4 / 8 / 16 / 32.
 * res2 of a bf16 R-50 / R-101 step with STRIDE_IN_1X1 exists only at the even rows and columns res3 reads (SYLPH_BK_STRIDED_TAIL, default
 * on): for stage 2 the tap then runs the dense launch of res2's last block from that block's input, which the step leaves intact, into a
 * buffer of its own (allocated on the first such call) and exports that -- the same values, the dense shape.  It changes nothing a later
 * tap, sylph_fcos_head or sylph_decode_nms reads and may be called any number of times, in any order with the other taps.
 * sylph_export_tower: conv output of layer `layer` of the cls (tower 0) / bbox (tower 1) tower on FPN level `level`
 * (sylph/modeling/meta_fcos/fcos.py:72-122,625-628) as (B,256,h_l,w_l) fp32 NCHW -- the value stored BEFORE GroupNorm when
 * the layer's GroupNorm is applied by its consumer -- and (coef_dev != NULL) that GroupNorm's per-(image, channel)
 * coefficients (a, b) with y = relu(a * x + b), as (B,256,2) fp32. */
int sylph_set_debug_taps(sylph_ctx* ctx, int on);
int sylph_export_stage(sylph_ctx* ctx, int stage, float* out_nchw_dev);
int sylph_export_tower(sylph_ctx* ctx, int tower, int layer, int level, float* y_nchw_dev, float* coef_dev);

/* Support-path taps: the output of one stage of the last sylph_codegen / sylph_codegen_classes / sylph_codegen_rois call on the
 * current batch (S support images or, after a ROI-list call, S = R ROIs; 49 ROI positions).  ROI, CONV_OUT and CONTEXT, the GroupNorm coefficients and the class tokens are always kept; the other
 * stages need sylph_set_debug_taps(1) before the first code-generator call of a batch shape, which copies each of them aside right
 * after the launch that writes it (same kernels and launches).  `index` numbers the layers of a stage:
 *   SYLPH_SUP_ROI          0: ROIAlign output, (S,256,7,7)
 *   SYLPH_SUP_GN_Y         GroupNorm layer: the conv output stored BEFORE its GroupNorm, (S,256,7,7)
 *   SYLPH_SUP_GN_COEF      GroupNorm layer: (a, b) per (image, channel) of its apply y = act(a * x + b), (S,256,2)
 *   SYLPH_SUP_LAYER_OUT    layer output after its GroupNorm and activation, (S,256,7,7)
 *   SYLPH_SUP_CONV_OUT     0: cls conv, (S,256,7,7); 1: the stacked 1-channel heads (bias, shot weight, class scale), (S,naux,7,7)
 *   SYLPH_SUP_CONTEXT      0: ROIEncoder context, (S,256,7,7)
 *   SYLPH_SUP_MSCAM        0: ROIEncoder box_pooler output after the MS-CAM gate, (S,256,7,7)
 *   SYLPH_SUP_TOKENS       0: tokens after the tokenizer FC stack, 1 + l: after encoder layer l, (S,256)
 *   SYLPH_SUP_CLS_TOKENS   0: class tokens (mean over the shots), (classes,256)
 * Layers: the code generator's tower layer i is index i; the ROIEncoder's box_pooler conv is 0 and tokenizer conv k is 1 + k.
 * All fp32 (maps NCHW).  sylph_support_tap_numel gives the element count of a tap; sylph_export_support writes it to out_dev. */
#define SYLPH_SUP_ROI 0
#define SYLPH_SUP_GN_Y 1
#define SYLPH_SUP_GN_COEF 2
#define SYLPH_SUP_LAYER_OUT 3
#define SYLPH_SUP_CONV_OUT 4
#define SYLPH_SUP_CONTEXT 5
#define SYLPH_SUP_MSCAM 6
#define SYLPH_SUP_TOKENS 7
#define SYLPH_SUP_CLS_TOKENS 8
int sylph_support_tap_numel(sylph_ctx* ctx, int stage, int index, int64_t* numel);
int sylph_export_support(sylph_ctx* ctx, int stage, int index, float* out_dev);

/* Kernel parity entry: ONE detectron2 BottleneckBlock (1x1 -> 3x3 -> 1x1, FrozenBN folded to scale/shift, identity or
 * projection shortcut, ReLU) through the same launches sylph_backbone_fpn uses for such a block (fused kernels included).
 * x (B,Cin,H,W) fp32 NCHW device; w_host[4] = conv1 (mid,Cin,1,1), conv2 (mid,mid,3,3), conv3 (cout,mid,1,1), shortcut
 * (cout,Cin,1,1) or NULL (identity block); scale_host / shift_host[4]: per-output-channel FrozenBN scale and shift of the
 * same four convs (host).  y (B,cout,Ho,Wo) fp32 NCHW device.  (call site meta_one_stage_detector.py:181,273) */
int sylph_bottleneck(sylph_ctx* ctx, const float* x_nchw_dev, int B, int Cin, int H, int W, int stride, int mid, int cout,
                     const float* const* w_host, const float* const* scale_host, const float* const* shift_host,
                     float* y_nchw_dev);
/* The same identity block (w_host[3] NULL) through the stride-2-output launch sylph_backbone_fpn uses for the last block of res2:
 * y (B,cout,H/2,W/2) holds the block's output at the even rows and columns, bit for bit what sylph_bottleneck gives there.  Only the
 * fused bf16 kernel's own shape (Cin = cout = 256, mid = 64) with even H and W; anything else is an error. */
int sylph_bottleneck_even(sylph_ctx* ctx, const float* x_nchw_dev, int B, int Cin, int H, int W, int mid, int cout,
                          const float* const* w_host, const float* const* scale_host, const float* const* shift_host,
                          float* y_nchw_dev);
/* Kernel parity entry: the res3 block-pair launch of sylph_backbone_fpn (SYLPH_BLOCK_PAIR) alone, bf16 contexts only.  Device inputs t2
 * (B,128,H,W) and x (B,512,H,W); host weights w3 (512,128), w1 (128,512) with their FrozenBN scale / shift.  Device outputs
 * y = relu(bn3(w3 t2) + x) (B,512,H,W) and t1 = relu(bn1(w1 y)) (B,128,H,W): conv3 + residual of one identity block and conv1 of the next. */
int sylph_res3_pair(sylph_ctx* ctx, const float* t2_nchw_dev, const float* x_nchw_dev, int B, int H, int W, const float* w3_host,
                    const float* s3_host, const float* b3_host, const float* w1_host, const float* s1_host, const float* b1_host,
                    float* y_nchw_dev, float* t1_nchw_dev);

/* Kernel parity entry: one FPN lateral as sylph_backbone_fpn launches it (detectron2 FPN.forward: lateral 1x1 conv + bias, plus
 * the nearest-2x upsampled level above, fused as a residual; call site meta_one_stage_detector.py:181,273).  x (B,C,H,W) fp32 NCHW
 * device; w_host (256,C,1,1), bias_host (256); top (B,256,H/2,W/2) device or NULL (fpn_lateral5); y (B,256,H,W) fp32 NCHW device. */
int sylph_fpn_lateral(sylph_ctx* ctx, const float* x_nchw_dev, int B, int C, int H, int W, const float* w_host, const float* bias_host,
                      const float* top_nchw_dev, float* y_nchw_dev);

/* Kernel parity entry: ONE grouped 3x3 conv (pad 1) with FrozenBN scale / shift and optional ReLU, as a ResNeXt bottleneck's conv2
 * launches it (conv_group.hip).  x (B,C,H,W) fp32 NCHW device; w_host (C, C / groups, 3, 3); scale / shift host (C); stride 1 or 2;
 * y (B,C,Ho,Wo) fp32 NCHW device.  C a multiple of 64, C / groups a power of two in [4, 64]. */
int sylph_group_conv(sylph_ctx* ctx, const float* x_nchw_dev, int B, int C, int H, int W, int groups, int stride, const float* w_host,
                     const float* scale_host, const float* shift_host, int relu, float* y_nchw_dev);
/* Kernel parity entry: ONE 3x3 stride-1 pad-1 conv 64 -> 64 channels with FrozenBN scale / shift, optional same-shape residual and
 * optional ReLU, as the res2 convs of a BasicBlock ResNet (R-18 / R-34) launch it: conv_rw64.hip in bf16 (SYLPH_CONV_RW64 = 0 off /
 * 1 auto / 2 always), the generic conv route otherwise (detectron2 BasicBlock.conv1 / conv2; call site
 * meta_one_stage_detector.py:181,273).  x, residual (or NULL), y (B,64,H,W) fp32 NCHW device; w_host (64,64,3,3); scale / shift host (64). */
int sylph_conv3x3_c64(sylph_ctx* ctx, const float* x_nchw_dev, int B, int H, int W, const float* w_host, const float* scale_host,
                      const float* shift_host, int relu, const float* residual_nchw_dev, float* y_nchw_dev);
/* Kernel parity entry: ONE detectron2 BasicBlock through the launches sylph_backbone_fpn makes for it:
 * t = relu(bn1(conv1 3x3 stride)(x)), y = relu(bn2(conv2 3x3)(t) + shortcut), shortcut = x or bn(conv 1x1 stride)(x).
 * w_host / scale_host / shift_host: conv1 (cout,Cin,3,3), conv2 (cout,cout,3,3), shortcut (cout,Cin,1,1) or NULL (then Cin == cout,
 * stride 1).  x (B,Cin,H,W), y (B,cout,Ho,Wo) fp32 NCHW device.  (Call site meta_one_stage_detector.py:181,273.) */
int sylph_basic_block(sylph_ctx* ctx, const float* x_nchw_dev, int B, int Cin, int H, int W, int stride, int cout,
                      const float* const* w_host, const float* const* scale_host, const float* const* shift_host, float* y_nchw_dev);
/* Kernel parity entry: ONE ResNeXt BottleneckBlock: sylph_bottleneck with a grouped conv2, w_host[1] (mid, mid / groups, 3, 3),
 * through the launches sylph_backbone_fpn makes for such a block. */
int sylph_bottleneck_grouped(sylph_ctx* ctx, const float* x_nchw_dev, int B, int Cin, int H, int W, int stride, int mid, int cout,
                             int groups, const float* const* w_host, const float* const* scale_host, const float* const* shift_host,
                             float* y_nchw_dev);

/* Kernel parity entry: ONE depthwise 3x3 conv (pad 1, stride 1 or 2, groups = C) as a MobileNetV2 block launches it (conv_dw.hip):
 * y = relu6(scale * dwconv(clamp(x, 0, 6)) + shift), fp32 arithmetic in every mode.  The clamp of the INPUT is the ReLU6 of the layer
 * in front, whose launch stores its result without it.  x (B,C,H,W), y (B,C,Ho,Wo) fp32 NCHW device; w_host (C,1,3,3); scale / shift host (C).
 * C a multiple of 8. */
int sylph_dwconv3x3(sylph_ctx* ctx, const float* x_nchw_dev, int B, int C, int H, int W, int stride, const float* w_host,
                    const float* scale_host, const float* shift_host, float* y_nchw_dev);
/* The channel count a MobileNetV2 tensor of C channels is computed with: C rounded up to the K slice of the implicit-GEMM kernels
 * (64 in SYLPH_BF16, 32 in the fp32 modes).  The pad channels are exactly zero in every tensor. */
int sylph_mbv2_padded_channels(sylph_ctx* ctx, int C);
/* Kernel parity entry: ONE MobileNetV2 InvertedResidual block (AdelaiDet mobilenet.py; call site meta_one_stage_detector.py:181,273)
 * through the launches sylph_backbone_fpn makes for it: t = 6: 1x1 expand Cin -> 6 Cin + FrozenBN + ReLU6, depthwise 3x3 (stride) +
 * FrozenBN + ReLU6, 1x1 project -> Cout + FrozenBN, + x when stride == 1 and Cin == Cout, nothing after the add; t = 1: no expand.
 * w_host / scale_host / shift_host[3] = expand (t Cin, Cin, 1, 1) or NULL (t = 1), depthwise (t Cin, 1, 3, 3), project (Cout, t Cin, 1, 1).
 * x (B,Cin,H,W) fp32 NCHW device; y (B,y_channels,Ho,Wo) with y_channels = Cout, or sylph_mbv2_padded_channels(Cout) to see the pad
 * channels too. */
int sylph_mbv2_block(sylph_ctx* ctx, const float* x_nchw_dev, int B, int Cin, int H, int W, int t, int Cout, int stride,
                     const float* const* w_host, const float* const* scale_host, const float* const* shift_host, int y_channels,
                     float* y_nchw_dev);

/* Bytes of device memory currently held by the context (weights + workspace). */
int64_t sylph_device_bytes(sylph_ctx* ctx);

/* Measurement aid (no reference counterpart; the reference only logs wall-clock s/img,
 * sylph/evaluation/meta_learn_evaluation.py:392-463): when enabled, every launch of the MFMA
 * implicit-GEMM conv kernel is bracketed by HIP events on the launch stream.  sylph_profile_read
 * synchronises the stream and returns the summed kernel time (ms), the algorithmic FLOPs
 * (2*M*N*K of the logical problem) and the number of launches since the previous read. */
int sylph_profile_enable(sylph_ctx* ctx, int on);
/* Kernel micro-benchmark (tuning aid): time `iters` back-to-back launches of one conv layer
 * (B images of HxW, Cin->Cout, KxK, random bf16/fp32 operands) with HIP events; ms per launch and the
 * algorithmic FLOPs of one launch are returned. */
int sylph_bench_conv(sylph_ctx* ctx, int B, int H, int W, int Cin, int Cout, int K, int stride, int pad, int has_res,
                     int relu, int with_gn, int iters, float* ms_out, double* flops_out);
int sylph_profile_read(sylph_ctx* ctx, double* conv_ms, double* conv_flops, int64_t* conv_launches);
/* The same records grouped by kernel (consumes them like sylph_profile_read): names_out = max_kernels x 64 bytes (NUL-terminated
 * kernel names in first-launch order), ms / flops / launches per kernel; *n_out kernels were written. */
int sylph_profile_read_kernels(sylph_ctx* ctx, int max_kernels, char* names_out, double* ms_out, double* flops_out,
                               int64_t* launches_out, int* n_out);
/* The conv route of every conv launch BUILT while profiling was enabled, in build order (consumes them): names_out = max_routes x 64
 * bytes, NUL-terminated "<kind> <BM>x<BN>[ nbuf<n>][ ks<k>]" with kind one of hpipe, igemm_halo, pw, spw, igemm_splitk, igemm
 * (e.g. "igemm_splitk 64x64 nbuf2 ks8"); *n_out routes were written.  A plan built once and replayed records its convs once. */
int sylph_conv_routes_read(sylph_ctx* ctx, int max_routes, char* names_out, int* n_out);

#ifdef __cplusplus
}
#endif
#endif /* SYLPH_HIP_H */
