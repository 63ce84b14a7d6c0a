"""ctypes binding of libsylph_hip.so (C ABI in include/sylph_hip.h).

The library is the ONLY compute path of this package: there is no eager/CPU fallback.  If the
shared object is missing or does not load, importing this module's ``lib()`` raises.
torch must be imported first so that the HIP runtime (libamdhip64.so.7) already loaded by torch is
the one the library binds to: device pointers are then shared between torch tensors and our kernels.
"""
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_float, c_int, c_int64, c_void_p

import torch  # noqa: F401  (loads the HIP runtime first)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SYLPH_LIB_PATH") or os.path.join(os.path.dirname(_HERE), "lib", "libsylph_hip.so")  # override: A/B kernel builds

SYLPH_F32 = 0
SYLPH_BF16 = 1
SYLPH_F32S = 2
# bounds of the COCO evaluation kernels (include/sylph_hip.h, csrc/kernels.h)
COCO_MATCH_TILE_GT = 128  # ground-truth boxes of one (image, category) pair whose IoU tile stays in LDS (maxDets[-1] <= 131; sylph_coco_match_tile_gt)
COCO_ACC_CHUNK = 1024  # rows of a category's segment per scan step
# bounds of the LVIS match kernel (include/sylph_hip.h, csrc/kernels.h)
LVIS_MATCH_SLICE_BYTES = 36 * 1024  # LDS of one wave = one pair: 32 D + G (8 D + 64) bytes fit, or the pair recomputes (sylph_lvis_match_fits)
LVIS_MATCH_MAX_DETS = 1024  # detections of one pair, i.e. max_dets_per_image


class SylphConfig(Structure):
    _fields_ = [
        ("resnet_depth", c_int), ("stride_in_1x1", c_int), ("num_cls_convs", c_int), ("num_box_convs", c_int),
        ("nlevels", c_int), ("strides", c_int * 8), ("pixel_mean", c_float * 3), ("pixel_std", c_float * 3),
        ("size_divisibility", c_int), ("use_scale", c_int), ("cond_use_bias", c_int),
        ("pre_nms_thresh", c_float), ("pre_nms_topk", c_int), ("nms_thresh", c_float), ("post_nms_topk", c_int),
        ("thresh_with_ctr", c_int), ("quality_mode", c_int),
        ("cg_tower_layers", c_int), ("cg_has_bias", c_int), ("cg_bias_l2_norm", c_int), ("cg_post_norm", c_int),
        ("cg_conv_l2_norm", c_int), ("cg_use_weight_scale", c_int), ("prior_prob", c_float), ("cand_cap", c_int),
        ("cg_type", c_int), ("tok_num_conv", c_int), ("tok_num_fc", c_int), ("enc_layers", c_int),
        ("head_num_fc", c_int), ("head_fc_dim", c_int), ("cg_meta_bias", c_int), ("cg_has_weight", c_int), ("cg_has_scale", c_int),
        ("num_share_convs", c_int), ("tower_norm", c_int), ("cg_tower_gn_mask", c_int), ("cg_tower_relu_mask", c_int),
        ("tower_deformable", c_int), ("num_groups", c_int), ("width_per_group", c_int),
        ("mobilenet", c_int), ("cg_code_ksize", c_int),
    ]


# name -> (restype, argtypes); every symbol declared in include/sylph_hip.h
PROTOTYPES = {
    "sylph_config_default": (None, [POINTER(SylphConfig)]),
    "sylph_ctx_create": (c_int, [c_int, c_int, POINTER(c_void_p)]),
    "sylph_ctx_destroy": (None, [c_void_p]),
    "sylph_last_error": (c_char_p, []),
    "sylph_set_stream": (c_int, [c_void_p, c_void_p]),
    "sylph_set_config": (c_int, [c_void_p, POINTER(SylphConfig)]),
    "sylph_load_weight": (c_int, [c_void_p, c_char_p, c_void_p, POINTER(c_int64), c_int]),
    "sylph_finalize_weights": (c_int, [c_void_p]),
    "sylph_preprocess": (c_int, [c_void_p, c_int, POINTER(c_void_p), POINTER(c_int), POINTER(c_int),
                                 POINTER(c_int), POINTER(c_int)]),
    "sylph_preprocess_u8": (c_int, [c_void_p, c_int, POINTER(c_void_p), POINTER(c_int), POINTER(c_int), POINTER(c_int),
                                    POINTER(c_int), c_int, POINTER(c_int), POINTER(c_int)]),
    "sylph_preprocess_views": (c_int, [c_void_p, c_int, POINTER(c_void_p)] + [POINTER(c_int)] * 9 + [c_int, POINTER(c_int), POINTER(c_int)]),
    "sylph_export_input": (c_int, [c_void_p, c_void_p]),
    "sylph_backbone_fpn": (c_int, [c_void_p]),
    "sylph_import_pyramid": (c_int, [c_void_p, c_int, c_int, c_int, POINTER(c_int), POINTER(c_int),
                                     POINTER(c_void_p)]),
    "sylph_export_pyramid": (c_int, [c_void_p, c_int, c_void_p]),
    "sylph_fcos_head": (c_int, [c_void_p, c_void_p, c_void_p, c_int]),
    "sylph_fcos_head_episodes": (c_int, [c_void_p, c_int, c_void_p, c_void_p, POINTER(c_int), POINTER(c_int)]),
    "sylph_fcos_head_codesets": (c_int, [c_void_p, c_int, c_void_p, c_void_p, POINTER(c_int)]),
    "sylph_fcos_head_pretrained": (c_int, [c_void_p, POINTER(c_int)]),
    "sylph_export_head": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sylph_import_head": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sylph_fcos_towers": (c_int, [c_void_p]),
    "sylph_record_store": (c_int, [c_void_p, POINTER(c_void_p)]),
    "sylph_record_load": (c_int, [c_void_p, c_void_p]),
    "sylph_record_info": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int64)]),
    "sylph_record_destroy": (None, [c_void_p, c_void_p]),
    "sylph_fcos_targets": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, POINTER(c_float), c_int, c_int, c_float, c_void_p, c_void_p]),
    "sylph_cls_grad_bytes": (c_int, [c_void_p, c_int, POINTER(c_int64)]),
    "sylph_cls_grad": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sylph_box_samples": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, POINTER(c_float), c_int, c_int, c_float, c_int] + [c_void_p] * 5),
    "sylph_box_grad_bytes": (c_int, [c_void_p, c_int, POINTER(c_int64)]),
    "sylph_box_grad": (c_int, [c_void_p, c_int] + [c_void_p] * 6 + [c_int, c_int] + [c_void_p] * 7),
    "sylph_box_branch_shape": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int), POINTER(ctypes.c_uint64)]),
    "sylph_get_box_branch": (c_int, [c_void_p, POINTER(c_float), POINTER(c_float), POINTER(c_float)]),
    "sylph_set_box_branch": (c_int, [c_void_p, POINTER(c_float), POINTER(c_float), POINTER(c_float)]),
    "sylph_roi_rows": (c_int, [c_void_p, c_int, c_void_p, POINTER(c_int), c_void_p]),
    "sylph_codegen_param_layout": (c_int, [c_void_p, c_int, ctypes.c_char_p, POINTER(c_int64), POINTER(c_int64), POINTER(c_int), POINTER(c_int64)]),
    "sylph_get_code_generator": (c_int, [c_void_p, POINTER(c_float)]),
    "sylph_set_code_generator": (c_int, [c_void_p, POINTER(c_float)]),
    "sylph_codegen_stamp": (c_int, [c_void_p, POINTER(ctypes.c_uint64)]),
    "sylph_codegen_train_bytes": (c_int, [c_void_p, c_int, c_int, POINTER(c_int64)]),
    "sylph_codegen_train_shape": (c_int, [c_void_p, c_int, c_int, POINTER(c_int), POINTER(c_int), POINTER(c_int64)]),
    "sylph_codegen_train_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, POINTER(c_int), c_int, POINTER(c_int), c_void_p, c_void_p]),
    "sylph_codegen_train_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sylph_roi_align": (c_int, [c_void_p, c_void_p, c_void_p]),
    "sylph_roi_align_rois": (c_int, [c_void_p, c_int, c_void_p, POINTER(c_int), c_void_p]),
    "sylph_decode_nms": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int), c_int, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sylph_decode_nms_codesets": (c_int, [c_void_p, c_int, POINTER(c_int), POINTER(c_int), c_int, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sylph_merge_views": (c_int, [c_void_p, c_int, c_int, POINTER(c_int), POINTER(c_float), POINTER(c_float), POINTER(c_float), POINTER(c_int),
                                  c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int] + [c_void_p] * 7),
    "sylph_merge_views_large_bytes": (c_int64, [c_int, c_int, c_int]),
    "sylph_merge_views_large": (c_int, [c_void_p, c_int, c_int, POINTER(c_int), POINTER(c_float), POINTER(c_float), POINTER(c_float), POINTER(c_int),
                                        c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int] + [c_void_p] * 8 + [c_int64]),
    "sylph_stitch_views_bytes": (c_int64, [c_int, c_int, c_int]),
    "sylph_stitch_views": (c_int, [c_void_p, c_int, c_int, POINTER(c_int), POINTER(c_float), POINTER(c_float), POINTER(c_float), POINTER(c_float),
                                   POINTER(c_int), POINTER(c_float), POINTER(c_float), c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float,
                                   c_float, c_int, c_int] + [c_void_p] * 9 + [c_int64]),
    "sylph_coco_match_tile_gt": (c_int, [c_int]),
    "sylph_coco_match": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int] + [c_void_p] * 5 + [c_int, c_int, c_void_p, c_int, c_void_p, c_int] +
                         [c_void_p] * 4),
    "sylph_coco_accumulate": (c_int, [c_void_p, c_int] + [c_void_p] * 4 + [c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int] +
                              [c_void_p] * 4),
    "sylph_lvis_match_fits": (c_int, [c_int, c_int]),
    "sylph_lvis_match": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int] + [c_void_p] * 7 + [c_int, c_int, c_void_p, c_int, c_void_p,
                                                                                                      c_int] + [c_void_p] * 4),
    "sylph_codegen": (c_int, [c_void_p, c_void_p, c_void_p]),
    "sylph_codegen_classes": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "sylph_codegen_rois": (c_int, [c_void_p, c_int, c_void_p, POINTER(c_int), c_int, POINTER(c_int), c_void_p]),
    "sylph_shot_row_floats": (c_int, [c_void_p, POINTER(c_int)]),
    "sylph_codegen_shots": (c_int, [c_void_p, c_int, c_void_p, POINTER(c_int), c_void_p]),
    "sylph_shot_combine": (c_int, [c_void_p, c_void_p, c_int, c_int, POINTER(c_int), c_int, POINTER(c_int), c_void_p, c_void_p]),
    "sylph_roi_table_uploads": (c_int, [c_void_p, POINTER(c_int64)]),
    "sylph_codegen_weight_norm": (c_int, [c_void_p, c_void_p]),
    "sylph_normalize_codes": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "sylph_reduce_codes": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int]),
    "sylph_conv2d": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int,
                             c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "sylph_group_norm": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "sylph_stem_maxpool": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sylph_set_debug_taps": (c_int, [c_void_p, c_int]),
    "sylph_export_stage": (c_int, [c_void_p, c_int, c_void_p]),
    "sylph_export_tower": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "sylph_support_tap_numel": (c_int, [c_void_p, c_int, c_int, POINTER(c_int64)]),
    "sylph_export_support": (c_int, [c_void_p, c_int, c_int, c_void_p]),
    "sylph_bottleneck": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, POINTER(c_void_p),
                                 POINTER(c_void_p), POINTER(c_void_p), c_void_p]),
    "sylph_bottleneck_even": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, POINTER(c_void_p),
                                      POINTER(c_void_p), POINTER(c_void_p), c_void_p]),
    "sylph_res3_pair": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int] + [c_void_p] * 8),
    "sylph_allgather_codes": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "sylph_comm_unique_id": (c_int, [ctypes.c_char_p]),
    "sylph_comm_init_rank": (c_int, [c_void_p, ctypes.c_char_p, c_int, c_int, POINTER(c_void_p)]),
    "sylph_comm_destroy": (c_int, [c_void_p]),
    "sylph_fpn_lateral": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sylph_group_conv": (c_int, [c_void_p, c_void_p] + [c_int] * 6 + [c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "sylph_bottleneck_grouped": (c_int, [c_void_p, c_void_p] + [c_int] * 8 + [POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p),
                                                                            c_void_p]),
    "sylph_conv3x3_c64": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "sylph_basic_block": (c_int, [c_void_p, c_void_p] + [c_int] * 6 + [POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p), c_void_p]),
    "sylph_dwconv3x3": (c_int, [c_void_p, c_void_p] + [c_int] * 5 + [c_void_p, c_void_p, c_void_p, c_void_p]),
    "sylph_mbv2_padded_channels": (c_int, [c_void_p, c_int]),
    "sylph_mbv2_block": (c_int, [c_void_p, c_void_p] + [c_int] * 7 + [POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p), c_int, c_void_p]),
    "sylph_device_bytes": (c_int64, [c_void_p]),
    "sylph_profile_enable": (c_int, [c_void_p, c_int]),
    "sylph_bench_conv": (c_int, [c_void_p] + [c_int] * 12 + [POINTER(c_float), POINTER(ctypes.c_double)]),
    "sylph_profile_read": (c_int, [c_void_p, POINTER(ctypes.c_double), POINTER(ctypes.c_double), POINTER(c_int64)]),
    "sylph_profile_read_kernels": (c_int, [c_void_p, c_int, ctypes.c_char_p, POINTER(ctypes.c_double), POINTER(ctypes.c_double),
                                           POINTER(c_int64), POINTER(c_int)]),
    "sylph_conv_routes_read": (c_int, [c_void_p, c_int, ctypes.c_char_p, POINTER(c_int)]),
}

_LIB = None


def lib():
    """Load libsylph_hip.so (once).  Raises if the HIP extension has not been built."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; "
                "g.build()' or make -C sylph-few-shot-detection_amd/csrc).  There is no CPU fallback.")
        _LIB = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(_LIB, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
    return _LIB


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().sylph_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"libsylph_hip {what}: {msg}")
