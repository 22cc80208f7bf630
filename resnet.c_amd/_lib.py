"""ctypes binding of librn_hip.so (the C-ABI of include/rn_hip.h).

The library is the product: if it is missing, or an entry point is missing
from it, loading fails loudly.  There is no CPU fallback anywhere in this
package.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# RN_HIP_LIB: another build of the same library (A/B timing of kernel changes)
LIB_PATH = os.environ.get("RN_HIP_LIB") or os.path.join(_HERE, "librn_hip.so")

RN_OK = 0
RN_ERR_INVALID, RN_ERR_HIP, RN_ERR_IO, RN_ERR_NOMEM, RN_ERR_UNSUPPORTED = 1, 2, 3, 4, 5
RN_LAYOUT_NCHW, RN_LAYOUT_NHWC = 0, 1
RN_FWD_REFERENCE_OPS, RN_FWD_FUSED = 0, 1
RN_DTYPE_F32, RN_DTYPE_BF16 = 0, 1
RN_CONV_MAX_DILATION = 1024  # the largest dilation of the rn_conv2d_dilated_* entry points

u64 = c_uint64
fptr = c_void_p  # device pointers travel as plain addresses


class ConvSecond(ctypes.Structure):
    _fields_ = [("inp", c_void_p), ("in_channels", c_uint64), ("H", c_uint64), ("W", c_uint64),
                ("stride", c_uint64)]


class ModelOutputs(ctypes.Structure):
    """rn_model_outputs: device pointers, any may be NULL; k = 0 means no top-k."""
    _fields_ = [("logits", c_void_p), ("features", c_void_p), ("probs", c_void_p), ("topk_prob", c_void_p),
                ("topk_idx", c_void_p), ("k", c_uint64)]


class ModelMaps(ctypes.Structure):
    """rn_model_maps: device pointers of the [B,C,H,W] fp32 maps behind layer1..layer4; NULL = not wanted."""
    _fields_ = [("layer", c_void_p * 4)]


class SegOutputs(ctypes.Structure):
    """rn_seg_outputs: device pointers of the label map [B,H,W] (bytes) and the scores [B,classes,H,W] fp32."""
    _fields_ = [("labels", c_void_p), ("scores", c_void_p)]


class FpnOutputs(ctypes.Structure):
    """rn_fpn_outputs: device pointers of the [B,a,H,W] fp32 levels 0..n-1, then the pooled one; NULL = not wanted."""
    _fields_ = [("level", c_void_p * 5)]


class RoiPool(ctypes.Structure):
    """rn_roi_pool: the RoIs (device [K,5]), the image size, the neck's levels the pooler reads, its parameters and
    the outputs pooled [K,a,PH,PW] fp32 and levels_out int32 [K] (or NULL)."""
    _fields_ = [("rois_dev", c_void_p), ("K", c_uint64), ("image_h", c_uint64), ("image_w", c_uint64),
                ("n_levels", c_int), ("level", c_int * 4), ("PH", c_uint64), ("PW", c_uint64),
                ("sampling_ratio", c_int), ("aligned", c_int), ("canonical_scale", c_double),
                ("canonical_level", c_int), ("pooled", c_void_p), ("levels_out", c_void_p)]


class RpnCandidates(ctypes.Structure):
    """rn_rpn_candidates: device pointers per (image, level, rank): index int32, logit, box [..,4], valid bytes, and
    count int32 [B,L]; any may be NULL where the entry point says so."""
    _fields_ = [("index", c_void_p), ("logit", c_void_p), ("box", c_void_p), ("valid", c_void_p), ("count", c_void_p)]


class RpnProposals(ctypes.Structure):
    """rn_rpn_proposals: device pointers of boxes [B,post,4], logits, levels int32, count int32 [B], rois [B*post,5]
    and cand_keep bytes [B,L,pre]; any may be NULL, not all."""
    _fields_ = [("boxes", c_void_p), ("logits", c_void_p), ("levels", c_void_p), ("count", c_void_p),
                ("rois", c_void_p), ("cand_keep", c_void_p)]


class RpnRequest(ctypes.Structure):
    """rn_rpn_request: the parameters, the proposals' outputs and the optional pre-NMS candidates"""
    _fields_ = [("pre_nms_top_n", c_uint64), ("post_nms_top_n", c_uint64), ("nms_thresh", c_float), ("logit_thresh", c_float),
                ("min_size", c_float), ("out", RpnProposals), ("cand", RpnCandidates)]


class Detections(ctypes.Structure):
    """rn_detections: device pointers of boxes [B,D,4], scores [B,D], labels and roi int32 [B,D], count int32 [B] (any may
    be NULL, not all five) and the optional intermediates probs [K,C], class_boxes [K,C,4], valid and keep bytes [K,C]."""
    _fields_ = [("boxes", c_void_p), ("scores", c_void_p), ("labels", c_void_p), ("roi", c_void_p), ("count", c_void_p),
                ("probs", c_void_p), ("class_boxes", c_void_p), ("valid", c_void_p), ("keep", c_void_p)]


class DetectRequest(ctypes.Structure):
    """rn_detect_request: the thresholds, detections_per_img, the decode's weights and the outputs"""
    _fields_ = [("score_thresh", c_float), ("nms_thresh", c_float), ("min_size", c_float), ("detections_per_img", c_uint64),
                ("weights", c_float * 4), ("out", Detections)]


class MaskRequest(ctypes.Structure):
    """rn_mask_request: the mask pooler's levels and parameters, the threshold and the outputs rois [B*D,5], pooled
    [B*D,M,M,a], probs [B,D,2M,2M], masks [B,D,H,W] fp32 and bits [B,D,H,W] bytes (any may be NULL, not all of the last
    three)"""
    _fields_ = [("n_levels", c_int), ("level", c_int * 4), ("sampling_ratio", c_int), ("aligned", c_int),
                ("canonical_scale", c_double), ("canonical_level", c_int), ("threshold", c_float), ("rois", c_void_p),
                ("pooled", c_void_p), ("probs", c_void_p), ("masks", c_void_p), ("bits", c_void_p)]


class KeypointRequest(ctypes.Structure):
    """rn_keypoint_request: the keypoint pooler's levels and parameters and the outputs rois [B*D,5], pooled [B*D,M,M,a],
    heat [B,D,Kp,4M,4M], keypoints [B,D,Kp,3] and scores [B,D,Kp] (any may be NULL, not all of the last three; keypoints
    and scores come together)"""
    _fields_ = [("n_levels", c_int), ("level", c_int * 4), ("sampling_ratio", c_int), ("aligned", c_int),
                ("canonical_scale", c_double), ("canonical_level", c_int), ("rois", c_void_p), ("pooled", c_void_p),
                ("heat", c_void_p), ("keypoints", c_void_p), ("scores", c_void_p)]


class Epilogue(ctypes.Structure):
    _fields_ = [("scale", c_void_p), ("shift", c_void_p), ("residual", c_void_p),
                ("relu", c_int)]


# name -> (restype, argtypes); every symbol include/rn_hip.h declares
SIGNATURES = {
    "rn_ctx_create": (c_int, [POINTER(c_void_p), c_int, c_void_p]),
    "rn_ctx_destroy": (c_int, [c_void_p]),
    "rn_ctx_set_layout": (c_int, [c_void_p, c_int]),
    "rn_ctx_get_layout": (c_int, [c_void_p]),
    "rn_ctx_set_sync_each_op": (c_int, [c_void_p, c_int]),
    "rn_ctx_set_deferred": (c_int, [c_void_p, c_int]),
    "rn_ctx_get_deferred": (c_int, [c_void_p]),
    "rn_flush": (c_int, [c_void_p]),
    "rn_observe": (c_int, [c_void_p, c_void_p]),
    "rn_ctx_deferred_stats": (c_int, [c_void_p] + [POINTER(u64)] * 5),
    "rn_ctx_set_weight_cache": (c_int, [c_void_p, c_int]),
    "rn_ctx_launch_count": (u64, [c_void_p]),
    "rn_conv_tile_candidates": (c_int, []),
    "rn_ctx_set_conv_tile": (c_int, [c_void_p, c_int]),
    "rn_ctx_set_split_k": (c_int, [c_void_p, c_int]),
    "rn_ctx_set_stem_items": (c_int, [c_void_p, c_int]),
    "rn_ctx_set_xcd_groups": (c_int, [c_void_p, c_int]),
    "rn_ctx_set_nchw_taps": (c_int, [c_void_p, c_int]),
    "rn_ctx_set_tap_skip": (c_int, [c_void_p, c_int]),
    "rn_ctx_tap_skip_stats": (c_int, [c_void_p, POINTER(u64), POINTER(u64)]),
    "rn_conv_tap_skip_plan": (c_int, [c_int] + [u64] * 9 + [c_int] + [POINTER(u64)] * 3 + [POINTER(c_int)]),
    "rn_ctx_set_debug_stamps": (c_int, [c_void_p, c_void_p]),
    "rn_ctx_stream": (c_void_p, [c_void_p]),
    "rn_ctx_device": (c_int, [c_void_p]),
    "rn_sync": (c_int, [c_void_p]),
    "rn_last_error": (c_char_p, [c_void_p]),
    "rn_status_string": (c_char_p, [c_int]),
    "rn_device_count": (c_int, [POINTER(c_int)]),
    "rn_device_locality": (c_int, [c_int, c_char_p, u64, POINTER(c_int), c_char_p, u64]),
    "rn_version": (c_char_p, []),
    "rn_malloc": (c_int, [c_void_p, POINTER(c_void_p), u64]),
    "rn_free": (c_int, [c_void_p, c_void_p]),
    "rn_memcpy_h2d": (c_int, [c_void_p, c_void_p, c_void_p, u64]),
    "rn_memcpy_d2h": (c_int, [c_void_p, c_void_p, c_void_p, u64]),
    "rn_memcpy_d2d": (c_int, [c_void_p, c_void_p, c_void_p, u64]),
    "rn_memset": (c_int, [c_void_p, c_void_p, c_int, u64]),
    "rn_load_f32_file": (c_int, [c_void_p, c_char_p, POINTER(c_void_p), POINTER(u64)]),
    "rn_save_f32_file": (c_int, [c_void_p, c_char_p, c_void_p, u64]),
    "rn_event_create": (c_int, [c_void_p, POINTER(c_void_p)]),
    "rn_event_destroy": (c_int, [c_void_p]),
    "rn_event_record": (c_int, [c_void_p, c_void_p]),
    "rn_event_elapsed_ms": (c_int, [c_void_p, c_void_p, POINTER(c_float)]),
    "rn_conv_output_size": (u64, [u64, u64, u64, u64]),
    "rn_conv2d_forward": (c_int, [c_void_p, fptr, fptr, fptr] + [u64] * 10),
    "rn_maxpool2d_forward": (c_int, [c_void_p, fptr, fptr] + [u64] * 9),
    "rn_avgpool2d_forward": (c_int, [c_void_p, fptr, fptr] + [u64] * 9),
    "rn_linear_forward": (c_int, [c_void_p, fptr, fptr, fptr, fptr] + [u64] * 3),
    "rn_relu_forward": (c_int, [c_void_p, fptr, fptr, u64]),
    "rn_batchnorm2d_forward": (c_int, [c_void_p] + [fptr] * 6 + [u64] * 3),
    "rn_add_forward": (c_int, [c_void_p, fptr, fptr, fptr, u64]),
    "rn_argmax_forward": (c_int, [c_void_p, fptr, c_void_p, u64, u64]),
    "rn_softmax_forward": (c_int, [c_void_p, fptr, fptr, u64, u64]),
    "rn_topk_forward": (c_int, [c_void_p, fptr, fptr, c_void_p, u64, u64, u64]),
    "rn_softmax_topk_forward": (c_int, [c_void_p, fptr, fptr, fptr, c_void_p, u64, u64, u64]),
    "rn_nchw_to_nhwc": (c_int, [c_void_p, fptr, fptr] + [u64] * 4),
    "rn_nhwc_to_nchw": (c_int, [c_void_p, fptr, fptr] + [u64] * 4),
    "rn_nhwc_to_nchw_dt": (c_int, [c_void_p, c_int, fptr, fptr] + [u64] * 4),
    "rn_conv2d_input_channels": (u64, [u64]),
    "rn_nchw_to_nhwc_pad": (c_int, [c_void_p, fptr, fptr] + [u64] * 5),
    "rn_conv2d_packed_weight_numel": (u64, [u64, u64, u64]),
    "rn_conv2d_pack_weight": (c_int, [c_void_p, fptr, fptr, u64, u64, u64]),
    "rn_batchnorm2d_fold": (c_int, [c_void_p] + [fptr] * 6 + [u64]),
    "rn_conv2d_nhwc_forward": (c_int, [c_void_p, fptr, fptr, fptr] + [u64] * 10
                               + [POINTER(Epilogue)]),
    "rn_conv2d_packed_weight_numel_dt": (u64, [c_int, u64, u64, u64]),
    "rn_conv2d_pack_weight_dt": (c_int, [c_void_p, c_int, fptr, fptr, u64, u64, u64]),
    "rn_nchw_to_nhwc_pad_dt": (c_int, [c_void_p, c_int, fptr, fptr] + [u64] * 6),
    "rn_image_u8_to_nhwc_pad_dt": (c_int, [c_void_p, c_int, c_void_p, c_void_p] + [u64] * 5
                                   + [POINTER(c_float), POINTER(c_float)]),
    "rn_resize_crop_geometry": (c_int, [u64] * 4 + [POINTER(u64)] * 4),
    "rn_resize_coefficients": (c_int, [u64] * 4 + [c_void_p, c_void_p, u64, POINTER(u64)]),
    "rn_image_u8_resize_crop": (c_int, [c_void_p, c_void_p, POINTER(u64), POINTER(u64), POINTER(u64), u64,
                                        c_void_p, u64, u64]),
    "rn_image_u8_resize_crop_table": (c_int, [POINTER(u64), POINTER(u64), POINTER(u64), u64, u64, u64, c_void_p,
                                              u64, POINTER(u64)]),
    "rn_image_u8_resize_crop_launch": (c_int, [c_void_p, c_void_p, c_void_p, u64, c_void_p, u64]),
    "rn_conv2d_nhwc_forward_dt": (c_int, [c_void_p, c_int, c_int, fptr, fptr, fptr] + [u64] * 10
                                  + [POINTER(Epilogue)]),
    "rn_conv2d_grouped_forward": (c_int, [c_void_p, fptr, fptr, fptr] + [u64] * 11),
    "rn_conv2d_grouped_packed_weight_numel_dt": (u64, [c_int, u64, u64, u64, u64]),
    "rn_conv2d_grouped_pack_weight_dt": (c_int, [c_void_p, c_int, fptr, fptr, u64, u64, u64, u64]),
    "rn_conv2d_grouped_nhwc_forward_dt": (c_int, [c_void_p, c_int, c_int, fptr, fptr, fptr] + [u64] * 11
                                          + [POINTER(Epilogue)]),
    "rn_conv_output_size_dilated": (u64, [u64, u64, u64, u64, u64]),
    "rn_conv2d_dilated_forward": (c_int, [c_void_p, fptr, fptr, fptr] + [u64] * 12),
    "rn_conv2d_dilated_nhwc_forward_dt": (c_int, [c_void_p, c_int, c_int, fptr, fptr, fptr] + [u64] * 12
                                          + [POINTER(Epilogue)]),
    "rn_conv2d_packed_weight_numel_exact": (u64, [u64, u64, u64]),
    "rn_conv2d_pack_weight_exact": (c_int, [c_void_p, fptr, fptr, u64, u64, u64]),
    "rn_conv2d_nhwc_exact_forward": (c_int, [c_void_p, fptr, fptr, fptr] + [u64] * 9
                                     + [POINTER(Epilogue)]),
    "rn_conv2d_packed_pair_weight_numel": (u64, [u64, u64, u64, u64]),
    "rn_conv2d_pack_weight_pair_dt": (c_int, [c_void_p, c_int, fptr, fptr, fptr, fptr, fptr]
                                      + [u64] * 4),
    "rn_conv2d_nhwc_pair_forward_dt": (c_int, [c_void_p, c_int, c_int, fptr, fptr, fptr] + [u64] * 10
                                       + [POINTER(ConvSecond), POINTER(Epilogue)]),
    "rn_model_set_pair_fusion": (c_int, [c_void_p, c_int]),
    "rn_model_set_stem_exact": (c_int, [c_void_p, c_int]),
    "rn_stem_pool_packed_weight_numel": (u64, [c_int]),
    "rn_stem_pool_pack_weight_dt": (c_int, [c_void_p, c_int, fptr, fptr, u64]),
    "rn_stem_pool_forward_dt": (c_int, [c_void_p, c_int, fptr, fptr, fptr, fptr, fptr, c_int, u64, u64, u64]),
    "rn_stem_pool_nchw_forward_dt": (c_int, [c_void_p, c_int, fptr, fptr, fptr, fptr, fptr, c_int, u64, u64, u64, u64]),
    "rn_stem_conv_pool_nchw_forward": (c_int, [c_void_p] + [fptr] * 6 + [u64] * 4),
    "rn_conv_chain_forward_dt": (c_int, [c_void_p, c_int] + [fptr] * 10 + [u64] * 4),
    "rn_conv_chain_pair_forward_dt": (c_int, [c_void_p, c_int] + [fptr] * 9 + [u64] * 5),
    "rn_model_set_chain": (c_int, [c_void_p, c_int]),
    "rn_model_set_stem_pool_fusion": (c_int, [c_void_p, c_int]),
    "rn_model_set_streams": (c_int, [c_void_p, c_int]),
    "rn_model_get_streams": (c_int, [c_void_p]),
    "rn_model_parts": (c_int, [c_void_p, u64]),
    "rn_model_set_front_parts": (c_int, [c_void_p, c_int]),
    "rn_maxpool2d_nhwc_forward_dt": (c_int, [c_void_p, c_int, fptr, fptr] + [u64] * 9),
    "rn_avgpool2d_nhwc_forward_dt": (c_int, [c_void_p, c_int, fptr, fptr] + [u64] * 9),
    "rn_global_avgpool_nhwc_forward_dt": (c_int, [c_void_p, c_int, fptr, fptr] + [u64] * 4),
    "rn_model_set_input_size": (c_int, [c_void_p, u64, u64]),
    "rn_model_input_size": (c_int, [c_void_p, POINTER(u64), POINTER(u64)]),
    "rn_model_max_sub_batch": (u64, [c_void_p]),
    "rn_model_set_dilation": (c_int, [c_void_p, c_int, c_int, c_int]),
    "rn_model_dilation": (c_int, [c_void_p, POINTER(c_int)]),
    "rn_model_output_stride": (c_int, [c_void_p]),
    "rn_model_create": (c_int, [c_void_p, POINTER(c_void_p), c_int]),
    "rn_model_create_ex": (c_int, [c_void_p, POINTER(c_void_p), c_int, c_int, c_int]),
    "rn_model_set_dtype": (c_int, [c_void_p, c_int]),
    "rn_model_set_classes": (c_int, [c_void_p, u64]),
    "rn_model_classes": (u64, [c_void_p]),
    "rn_model_features": (u64, [c_void_p]),
    "rn_model_forward_outputs": (c_int, [c_void_p, fptr, u64, POINTER(ModelOutputs), c_int]),
    "rn_model_forward_outputs_u8": (c_int, [c_void_p, c_void_p, u64, POINTER(ModelOutputs), c_int]),
    "rn_model_stage_shape": (c_int, [c_void_p, c_int, POINTER(u64), POINTER(u64), POINTER(u64)]),
    "rn_model_forward_maps": (c_int, [c_void_p, fptr, u64, POINTER(ModelOutputs), POINTER(ModelMaps), c_int]),
    "rn_model_forward_maps_u8": (c_int, [c_void_p, c_void_p, u64, POINTER(ModelOutputs), POINTER(ModelMaps), c_int]),
    "rn_upsample_bilinear_forward": (c_int, [c_void_p, fptr] + [u64] * 7 + [fptr, c_void_p]),
    "rn_seg_head_create": (c_int, [c_void_p, POINTER(c_void_p), u64, u64, u64]),
    "rn_concat_channels_forward_dt": (c_int, [c_void_p, c_int, u64, POINTER(c_void_p), POINTER(u64), c_void_p, u64,
                                              c_void_p, u64, u64]),
    "rn_seg_head_create_deeplab": (c_int, [c_void_p, POINTER(c_void_p), u64, u64, u64, u64, POINTER(u64)]),
    "rn_seg_head_set_center_tap": (c_int, [c_void_p, c_int]),
    "rn_seg_head_set_dtype": (c_int, [c_void_p, c_int]),
    "rn_seg_head_set_tensor": (c_int, [c_void_p, c_char_p, c_void_p, u64]),
    "rn_seg_head_finalize": (c_int, [c_void_p]),
    "rn_seg_head_destroy": (c_int, [c_void_p]),
    "rn_seg_head_forward": (c_int, [c_void_p, c_void_p] + [u64] * 5 + [fptr, c_void_p]),
    "rn_model_forward_segment": (c_int, [c_void_p, c_void_p, fptr, u64, POINTER(ModelOutputs), POINTER(SegOutputs),
                                         c_int]),
    "rn_model_forward_segment_u8": (c_int, [c_void_p, c_void_p, c_void_p, u64, POINTER(ModelOutputs),
                                            POINTER(SegOutputs), c_int]),
    "rn_upsample_nearest_add_forward_dt": (c_int, [c_void_p, c_int, c_void_p] + [u64] * 4 + [c_void_p, c_void_p, u64, u64]),
    "rn_fpn_create": (c_int, [c_void_p, POINTER(c_void_p), u64, POINTER(u64), u64, c_int]),
    "rn_fpn_set_dtype": (c_int, [c_void_p, c_int]),
    "rn_fpn_set_tensor": (c_int, [c_void_p, c_char_p, c_void_p, u64]),
    "rn_fpn_finalize": (c_int, [c_void_p]),
    "rn_fpn_destroy": (c_int, [c_void_p]),
    "rn_fpn_level_shape": (c_int, [c_void_p, c_int, u64, u64, POINTER(u64), POINTER(u64), POINTER(u64)]),
    "rn_fpn_forward": (c_int, [c_void_p, POINTER(c_void_p), u64, POINTER(u64), POINTER(u64), POINTER(c_void_p)]),
    "rn_model_forward_fpn": (c_int, [c_void_p, c_void_p, fptr, u64, POINTER(ModelOutputs), POINTER(c_int),
                                     POINTER(FpnOutputs), c_int]),
    "rn_model_forward_fpn_u8": (c_int, [c_void_p, c_void_p, c_void_p, u64, POINTER(ModelOutputs), POINTER(c_int),
                                        POINTER(FpnOutputs), c_int]),
    "rn_roi_level_thresholds": (c_int, [u64, POINTER(c_float), c_double, c_int, POINTER(c_float)]),
    "rn_roi_align_forward_dt": (c_int, [c_void_p, c_int, u64, POINTER(c_void_p), POINTER(u64), POINTER(u64), POINTER(c_float),
                                        POINTER(c_float), u64, u64, c_void_p, u64, u64, u64, c_int, c_int, c_void_p, c_void_p]),
    "rn_fpn_forward_rois": (c_int, [c_void_p, POINTER(c_void_p), u64, POINTER(u64), POINTER(u64), POINTER(c_void_p),
                                    POINTER(RoiPool)]),
    "rn_model_forward_rois": (c_int, [c_void_p, c_void_p, fptr, u64, POINTER(ModelOutputs), POINTER(c_int),
                                      POINTER(FpnOutputs), POINTER(RoiPool), c_int]),
    "rn_model_forward_rois_u8": (c_int, [c_void_p, c_void_p, c_void_p, u64, POINTER(ModelOutputs), POINTER(c_int),
                                         POINTER(FpnOutputs), POINTER(RoiPool), c_int]),
    "rn_rpn_select_decode_forward": (c_int, [c_void_p, u64, POINTER(c_void_p), u64, POINTER(u64), POINTER(u64), u64,
                                             POINTER(c_float), u64, u64, u64, c_float, c_float, POINTER(RpnCandidates)]),
    "rn_rpn_nms_merge_forward": (c_int, [c_void_p, POINTER(RpnCandidates), u64, u64, u64, u64, c_float,
                                         POINTER(RpnProposals)]),
    "rn_nms_forward": (c_int, [c_void_p, c_void_p, c_void_p, u64, u64, c_float, c_void_p, c_void_p]),
    "rn_box_decode_forward": (c_int, [c_void_p, fptr, fptr, u64] + [c_float] * 6 + [fptr]),
    "rn_rpn_create": (c_int, [c_void_p, POINTER(c_void_p), u64, u64, u64, POINTER(c_float)]),
    "rn_rpn_set_tensor": (c_int, [c_void_p, c_char_p, c_void_p, u64]),
    "rn_rpn_finalize": (c_int, [c_void_p]),
    "rn_rpn_destroy": (c_int, [c_void_p]),
    "rn_rpn_forward": (c_int, [c_void_p, POINTER(c_void_p), u64, POINTER(u64), POINTER(u64), u64, u64, POINTER(RpnRequest)]),
    "rn_fpn_forward_proposals": (c_int, [c_void_p, c_void_p, POINTER(c_void_p), u64, POINTER(u64), POINTER(u64),
                                         POINTER(c_void_p), u64, u64, POINTER(RpnRequest), POINTER(RoiPool)]),
    "rn_model_forward_proposals": (c_int, [c_void_p, c_void_p, c_void_p, fptr, u64, POINTER(ModelOutputs), POINTER(c_int),
                                           POINTER(FpnOutputs), POINTER(RpnRequest), POINTER(RoiPool), c_int]),
    "rn_model_forward_proposals_u8": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, u64, POINTER(ModelOutputs), POINTER(c_int),
                                              POINTER(FpnOutputs), POINTER(RpnRequest), POINTER(RoiPool), c_int]),
    "rn_detect_postprocess_forward": (c_int, [c_void_p, fptr, fptr, u64, u64, u64, u64, u64, POINTER(DetectRequest)]),
    "rn_box_head_create": (c_int, [c_void_p, POINTER(c_void_p), u64, u64, u64]),
    "rn_box_head_set_tensor": (c_int, [c_void_p, c_char_p, c_void_p, u64]),
    "rn_box_head_finalize": (c_int, [c_void_p]),
    "rn_box_head_destroy": (c_int, [c_void_p]),
    "rn_box_head_forward": (c_int, [c_void_p, fptr, fptr, u64, u64, u64, u64, POINTER(DetectRequest), fptr]),
    "rn_fpn_forward_detections": (c_int, [c_void_p, c_void_p, c_void_p, POINTER(c_void_p), u64, POINTER(u64), POINTER(u64),
                                          POINTER(c_void_p), u64, u64, POINTER(RpnRequest), POINTER(RoiPool),
                                          POINTER(DetectRequest)]),
    "rn_model_forward_detections": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, fptr, u64, POINTER(ModelOutputs),
                                            POINTER(c_int), POINTER(FpnOutputs), POINTER(RpnRequest), POINTER(RoiPool),
                                            POINTER(DetectRequest), c_int]),
    "rn_model_forward_detections_u8": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, u64, POINTER(ModelOutputs),
                                               POINTER(c_int), POINTER(FpnOutputs), POINTER(RpnRequest), POINTER(RoiPool),
                                               POINTER(DetectRequest), c_int]),
    "rn_roi_align_nhwc_forward_dt": (c_int, [c_void_p, c_int, u64, POINTER(c_void_p), POINTER(u64), POINTER(u64), POINTER(c_float),
                                             POINTER(c_float), u64, u64, c_void_p, u64, u64, u64, c_int, c_int, c_void_p,
                                             c_void_p]),
    "rn_detection_rois_forward": (c_int, [c_void_p, fptr, fptr, u64, u64, fptr]),
    "rn_mask_predict_forward": (c_int, [c_void_p, fptr, fptr, fptr, fptr, u64, u64, u64, u64, fptr]),
    "rn_paste_masks_forward": (c_int, [c_void_p, fptr, fptr, fptr, u64, u64, u64, u64, c_float, fptr, fptr]),
    "rn_mask_head_create": (c_int, [c_void_p, POINTER(c_void_p), u64, u64, POINTER(u64), u64, u64, u64]),
    "rn_mask_head_set_tensor": (c_int, [c_void_p, c_char_p, c_void_p, u64]),
    "rn_mask_head_finalize": (c_int, [c_void_p]),
    "rn_mask_head_destroy": (c_int, [c_void_p]),
    "rn_mask_head_forward": (c_int, [c_void_p, fptr, fptr, fptr, u64, u64, u64, POINTER(MaskRequest)]),
    "rn_fpn_forward_masks": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_void_p), u64, POINTER(u64), POINTER(u64),
                                     POINTER(c_void_p), u64, u64, POINTER(RpnRequest), POINTER(RoiPool),
                                     POINTER(DetectRequest), POINTER(MaskRequest)]),
    "rn_model_forward_masks": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, fptr, u64, POINTER(ModelOutputs),
                                       POINTER(c_int), POINTER(FpnOutputs), POINTER(RpnRequest), POINTER(RoiPool),
                                       POINTER(DetectRequest), POINTER(MaskRequest), c_int]),
    "rn_model_forward_masks_u8": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, u64, POINTER(ModelOutputs),
                                          POINTER(c_int), POINTER(FpnOutputs), POINTER(RpnRequest), POINTER(RoiPool),
                                          POINTER(DetectRequest), POINTER(MaskRequest), c_int]),
    "rn_keypoint_predict_forward": (c_int, [c_void_p, fptr, fptr, fptr, fptr, u64, u64, u64, u64, u64, fptr, fptr, fptr]),
    "rn_heatmaps_to_keypoints_forward": (c_int, [c_void_p, fptr, fptr, fptr, u64, u64, u64, u64, u64, fptr, fptr]),
    "rn_keypoint_head_create": (c_int, [c_void_p, POINTER(c_void_p), u64, u64, POINTER(u64), u64, u64]),
    "rn_keypoint_head_set_tensor": (c_int, [c_void_p, c_char_p, c_void_p, u64]),
    "rn_keypoint_head_finalize": (c_int, [c_void_p]),
    "rn_keypoint_head_destroy": (c_int, [c_void_p]),
    "rn_keypoint_head_forward": (c_int, [c_void_p, fptr, fptr, fptr, u64, u64, u64, POINTER(KeypointRequest)]),
    "rn_fpn_forward_keypoints": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_void_p), u64, POINTER(u64),
                                         POINTER(u64), POINTER(c_void_p), u64, u64, POINTER(RpnRequest), POINTER(RoiPool),
                                         POINTER(DetectRequest), POINTER(MaskRequest), POINTER(KeypointRequest)]),
    "rn_model_forward_keypoints": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, fptr, u64,
                                           POINTER(ModelOutputs), POINTER(c_int), POINTER(FpnOutputs), POINTER(RpnRequest),
                                           POINTER(RoiPool), POINTER(DetectRequest), POINTER(MaskRequest),
                                           POINTER(KeypointRequest), c_int]),
    "rn_model_forward_keypoints_u8": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, u64,
                                              POINTER(ModelOutputs), POINTER(c_int), POINTER(FpnOutputs), POINTER(RpnRequest),
                                              POINTER(RoiPool), POINTER(DetectRequest), POINTER(MaskRequest),
                                              POINTER(KeypointRequest), c_int]),
    "rn_model_destroy": (c_int, [c_void_p]),
    "rn_model_set_tensor": (c_int, [c_void_p, c_char_p, c_void_p, u64]),
    "rn_model_load_dir": (c_int, [c_void_p, c_char_p]),
    "rn_model_finalize": (c_int, [c_void_p]),
    "rn_model_tensor_key": (c_char_p, [c_void_p, u64, POINTER(u64)]),
    "rn_model_forward": (c_int, [c_void_p, fptr, u64, fptr, c_int]),
    "rn_model_forward_u8": (c_int, [c_void_p, c_void_p, u64, fptr, c_int]),
    "rn_model_forward_images_u8": (c_int, [c_void_p, c_void_p, POINTER(u64), POINTER(u64), POINTER(u64), u64, fptr,
                                           c_int]),
    "rn_model_tune": (c_int, [c_void_p, fptr, u64, fptr, c_int]),
    "rn_model_export_tuning": (c_int, [c_void_p, POINTER(u64), u64, POINTER(u64)]),
    "rn_model_import_tuning": (c_int, [c_void_p, POINTER(u64), u64]),
    "rn_model_set_profiling": (c_int, [c_void_p, c_int]),
    "rn_model_profile_count": (u64, [c_void_p]),
    "rn_model_profile_get": (c_int, [c_void_p, u64, POINTER(c_char_p), POINTER(c_char_p),
                                     POINTER(c_float), POINTER(c_double), POINTER(c_double)]),
    "rn_model_activation_bytes": (u64, [c_void_p]),
    "rn_model_capture": (c_int, [c_void_p, fptr, u64, fptr, c_int, POINTER(c_void_p)]),
    "rn_graph_launch": (c_int, [c_void_p]),
    "rn_graph_destroy": (c_int, [c_void_p]),
    "rn_graph_node_count": (u64, [c_void_p]),
    "rn_pipeline_create": (c_int, [c_void_p, POINTER(c_void_p), u64, c_int]),
    "rn_pipeline_destroy": (c_int, [c_void_p]),
    "rn_pipeline_input_buffer": (c_int, [c_void_p, POINTER(c_void_p)]),
    "rn_pipeline_submit": (c_int, [c_void_p, c_void_p]),
    "rn_pipeline_collect": (c_int, [c_void_p, c_void_p]),
    "rn_pipeline_in_flight": (u64, [c_void_p]),
    "rn_pipeline_submit_n": (c_int, [c_void_p, c_void_p, u64]),
    "rn_pipeline_collect_n": (c_int, [c_void_p, c_void_p, c_void_p, POINTER(u64)]),
    "rn_pipeline_create_u8": (c_int, [c_void_p, POINTER(c_void_p), u64, c_int]),
    "rn_pipeline_input_buffer_u8": (c_int, [c_void_p, POINTER(c_void_p)]),
    "rn_pipeline_submit_u8_n": (c_int, [c_void_p, c_void_p, u64]),
    "rn_pipeline_create_images_u8": (c_int, [c_void_p, POINTER(c_void_p), u64, c_int, u64]),
    "rn_pipeline_submit_images_u8_n": (c_int, [c_void_p, POINTER(c_void_p), POINTER(u64), POINTER(u64), u64]),
    "rn_shard_bounds": (None, [u64, c_int, c_int, POINTER(u64), POINTER(u64)]),
    "rn_shard_create": (c_int, [POINTER(c_void_p), POINTER(c_int), c_int, c_int]),
    "rn_shard_create_ex": (c_int, [POINTER(c_void_p), POINTER(c_int), c_int, c_int, c_int, c_int]),
    "rn_shard_destroy": (c_int, [c_void_p]),
    "rn_shard_count": (c_int, [c_void_p]),
    "rn_shard_last_error": (c_char_p, [c_void_p]),
    "rn_shard_set_tensor": (c_int, [c_void_p, c_char_p, c_void_p, u64]),
    "rn_shard_load_dir": (c_int, [c_void_p, c_char_p]),
    "rn_shard_set_dtype": (c_int, [c_void_p, c_int]),
    "rn_shard_finalize": (c_int, [c_void_p]),
    "rn_shard_forward": (c_int, [c_void_p, c_void_p, u64, c_void_p, c_void_p, c_int]),
    "rn_shard_tune": (c_int, [c_void_p, c_void_p, u64, c_int]),
    "rn_shard_model": (c_void_p, [c_void_p, c_int]),
    "rn_shard_placement": (c_int, [c_void_p, c_int, POINTER(c_int), POINTER(c_int), c_char_p, u64]),
    "rn_shard_stream_open": (c_int, [c_void_p, u64, c_int]),
    "rn_shard_stream_buffer": (c_int, [c_void_p, c_int, POINTER(c_void_p), POINTER(u64), POINTER(u64)]),
    "rn_shard_submit": (c_int, [c_void_p, c_void_p]),
    "rn_shard_collect": (c_int, [c_void_p, c_void_p, c_void_p]),
    "rn_shard_in_flight": (c_int, [c_void_p]),
    "rn_shard_stream_close": (c_int, [c_void_p]),
    "rn_shard_forward_u8": (c_int, [c_void_p, c_void_p, u64, c_void_p, c_void_p, c_int]),
    "rn_shard_stream_open_u8": (c_int, [c_void_p, u64, c_int]),
    "rn_shard_stream_buffer_u8": (c_int, [c_void_p, c_int, POINTER(c_void_p), POINTER(u64), POINTER(u64)]),
    "rn_shard_submit_u8": (c_int, [c_void_p, c_void_p]),
}

_lib = None


class RnError(RuntimeError):
    """A C-ABI call returned a non-zero status (the reference would have aborted:
    gpuAssert, cuda/helpers.cuh:13-22)."""

    def __init__(self, status: int, where: str, detail: str = ""):
        self.status = status
        super().__init__(f"{where}: status {status}" + (f" ({detail})" if detail else ""))


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` (or `make -C resnet.c_amd/csrc`). There is no CPU fallback.")
        # torch ships its own libamdhip64.so.7; importing it first makes this library
        # bind to the same HIP runtime instance instead of loading a second one.
        try:
            import torch  # noqa: F401
        except Exception:  # pragma: no cover - torch is plumbing, not required
            pass
        L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def source_digest() -> str:
    """sha256 (16 hex digits) over the sources librn_hip.so is built from: what a measurement of
    the kernels (a PMC pass, a trace) is stamped with, so that a later build can tell whether
    the figure still describes it.  (The GPU box has no .git; a commit id would also change with
    every documentation commit.)"""
    import glob
    import hashlib

    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(_HERE, "csrc", "*.hip")) + glob.glob(os.path.join(_HERE, "csrc", "*.h")) +
                   glob.glob(os.path.join(_HERE, "csrc", "*.c")) + glob.glob(os.path.join(_HERE, "csrc", "Makefile")) +
                   [os.path.join(os.path.dirname(_HERE), "include", "rn_hip.h")])
    for f in files:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def set_tensors(handle, prefix: str, ctx, shapes, state) -> None:
    """What every object behind the backbone does with its state dict: `prefix`_set_tensor for each key of the ordered
    {key: shape} `shapes` (state[key] as contiguous fp32, of that many elements), then `prefix`_finalize."""
    import numpy as np
    for key, shape in shapes.items():
        arr = np.ascontiguousarray(state[key], dtype=np.float32)
        assert arr.size == int(np.prod(shape)), (key, arr.shape, shape)
        check(getattr(lib(), prefix + "_set_tensor")(handle, key.encode(), arr.ctypes.data, arr.size),
              f"{prefix}_set_tensor({key})", ctx.handle)
    check(getattr(lib(), prefix + "_finalize")(handle), prefix + "_finalize", ctx.handle)


class Handle:
    """close() and __del__ of an object that owns the C handle self.handle; DESTROY names its destroy function."""
    DESTROY = ""
    handle = None

    def close(self) -> None:
        if self.handle:
            getattr(lib(), self.DESTROY)(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def check(status: int, where: str, ctx=None) -> None:
    if status != RN_OK:
        detail = ""
        if ctx:
            msg = lib().rn_last_error(ctx)
            detail = msg.decode() if msg else ""
        if not detail:
            detail = lib().rn_status_string(status).decode()
        raise RnError(status, where, detail)
