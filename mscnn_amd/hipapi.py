"""ctypes binding of libmscnn_hip.so (include/mscnn_hip.h) for Python callers.

Tensors are torch CUDA (ROCm) tensors; torch is used only as the device allocator and stream
owner -- every computation is done by the hand-written HIP kernels behind the C ABI.
There is no CPU fallback: a missing library or a host tensor raises.
"""
import ctypes as C
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmscnn_hip.so")
_lib = None


class MscnnError(RuntimeError):
    pass


class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("N", "Cin", "H", "W", "Cout", "Kh", "Kw", "pad_h", "pad_w",
                                       "stride_h", "stride_w", "group", "relu", "algo", "tune_variant", "tune_grid", "tune_flags")]


# mscnn_conv_algo
AMAX_SLOTS = 1024
ALGO_AUTO, ALGO_DIRECT, ALGO_WINO_F2, ALGO_WINO_F3, ALGO_F16, ALGO_WINO_F3_X3, ALGO_WINO_F4 = 0, 1, 2, 3, 4, 5, 6


MAX_HEADS = 16


class BoxOutputDesc(C.Structure):
    _fields_ = [("num_heads", C.c_int), ("num", C.c_int), ("channels", C.c_int),
                ("head_h", C.c_int * MAX_HEADS), ("head_w", C.c_int * MAX_HEADS),
                ("field_w", C.c_float * MAX_HEADS), ("field_h", C.c_float * MAX_HEADS),
                ("downsample_rate", C.c_float * MAX_HEADS),
                ("fg_thr", C.c_float), ("iou_thr", C.c_float), ("nms_mode", C.c_int),
                ("field_whr", C.c_float), ("field_xyr", C.c_float),
                ("max_nms_num", C.c_int), ("max_post_nms_num", C.c_int), ("min_size", C.c_float),
                ("do_bbox_norm", C.c_int), ("bbox_mean", C.c_float * 4), ("bbox_std", C.c_float * 4)]


class DetectionsDesc(C.Structure):
    _fields_ = [("ncls", C.c_int), ("cls_id", C.c_int), ("bbox_mean", C.c_float * 4), ("bbox_std", C.c_float * 4),
                ("proposal_thr", C.c_float), ("ratio_h", C.c_double), ("ratio_w", C.c_double),
                ("org_h", C.c_double), ("org_w", C.c_double), ("nms_overlap", C.c_double)]


class ProposalsDesc(C.Structure):
    """mscnn_proposals_desc (include/mscnn_hip.h): one per image."""
    _fields_ = [("proposal_thr", C.c_float), ("ratio_h", C.c_double), ("ratio_w", C.c_double)]


PROPOSALS_IMAGES_PER_LAUNCH = 64      # MSCNN_PROPOSALS_IMAGES_PER_LAUNCH


class NmsParams(C.Structure):
    """mscnn_nms_params (include/mscnn_hip.h): bbNms's type / ovrDnm / thr and the plain stage's det_thr."""
    _fields_ = [("type", C.c_int), ("ovr_dnm", C.c_int), ("thr", C.c_double), ("det_thr", C.c_float)]


NMS_MODES = {"IOU": 0, "IOMU": 1, "IOFU": 2}


def nms_params(type="maxg", ovr_dnm="union", thr=None, det_thr=0.0, maxn=None):
    """bbNms's knobs as the scripts spell them -> NmsParams (mscnn_nms_params_from_names: 'ms', 'cover', 'none', a finite maxn and
    out-of-range values are refused, naming the value).  thr None: bbNms's default, -inf."""
    out = NmsParams()
    _check(lib().mscnn_nms_params_from_names(None if type is None else str(type).encode(), None if ovr_dnm is None else str(ovr_dnm).encode(),
                                             float("-inf") if thr is None else float(thr), float("inf") if maxn is None else float(maxn),
                                             float(det_thr), C.byref(out)))
    return out


NMS_NULL = object()      # nms=NMS_NULL: the *_nms_fwd entry point with a NULL params pointer (nms=None: the entry point without params)


def _nms_ref(nms):
    """nms: NMS_NULL, an NmsParams or a dict of nms_params() keyword arguments -> the pointer argument (NMS_NULL: NULL)."""
    if nms is NMS_NULL:
        return None
    return C.byref(nms if isinstance(nms, NmsParams) else nms_params(**nms))


def lib():
    """Load libmscnn_hip.so; raises (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MscnnError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(LIB_PATH)
        L.mscnn_last_error.restype = C.c_char_p
        L.mscnn_version.restype = C.c_char_p
        L.mscnn_conv2d_plan_kernel.restype = C.c_char_p
        L.mscnn_conv2d_plan_kernel.argtypes = [C.c_void_p]
        L.mscnn_conv2d_plan_publishes_amax.argtypes = [C.c_void_p]
        L.mscnn_conv2d_plan_set_amax_io.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.mscnn_conv2d_plan_dtype.restype = C.c_char_p
        L.mscnn_conv2d_plan_dtype.argtypes = [C.c_void_p]
        L.mscnn_inner_product_f16_supported.argtypes = [C.c_int, C.c_int]
        L.mscnn_inner_product_x3_supported.argtypes = [C.c_int, C.c_int]
        L.mscnn_inner_product_x3_packed_bytes.restype = C.c_size_t
        L.mscnn_inner_product_x3_packed_bytes.argtypes = [C.c_int, C.c_int]
        L.mscnn_inner_product_x3_workspace_bytes.restype = C.c_size_t
        L.mscnn_inner_product_x3_workspace_bytes.argtypes = [C.c_int] * 3
        L.mscnn_inner_product_x3_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.mscnn_inner_product_x3_fwd.argtypes = [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.mscnn_inner_product_wg_supported.argtypes = [C.c_int] * 3
        L.mscnn_inner_product_wg_packed_bytes.restype = C.c_size_t
        L.mscnn_inner_product_wg_packed_bytes.argtypes = [C.c_int, C.c_int]
        L.mscnn_inner_product_wg_workspace_bytes.restype = C.c_size_t
        L.mscnn_inner_product_wg_workspace_bytes.argtypes = [C.c_int] * 3
        L.mscnn_inner_product_wg_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.mscnn_inner_product_wg_fwd.argtypes = [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p, C.c_size_t, C.c_void_p]
        L.mscnn_max_rel_diff_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p]
        L.mscnn_sum_squares_f32.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.mscnn_max_rel_diff_strided_f32.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_double,
                                                     C.c_void_p, C.c_void_p]
        L.mscnn_store_words_i32.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.mscnn_wgemm_handoff_event.restype = C.c_ulonglong
        L.mscnn_wgemm_handoff_event.argtypes = []
        L.mscnn_wgemm_force_whole_tiles.restype = None
        L.mscnn_wgemm_force_whole_tiles.argtypes = [C.c_int]
        L.mscnn_wgemm_whole_tiles_forced.argtypes = []
        L.mscnn_debug_inner_product_rows.restype = None
        L.mscnn_debug_inner_product_rows.argtypes = [C.c_int]
        L.mscnn_debug_wgemm_handoff_fault.restype = None
        L.mscnn_debug_wgemm_handoff_fault.argtypes = [C.c_int, C.c_uint]
        L.mscnn_inner_product_pack_f16.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.mscnn_inner_product_fwd_f16.argtypes = [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p]
        for f in ("mscnn_conv2d_plan_flops", "mscnn_conv2d_plan_executed_flops"):
            getattr(L, f).restype = C.c_double
            getattr(L, f).argtypes = [C.c_void_p]
        L.mscnn_conv2d_plan_set_profiling.argtypes = [C.c_void_p, C.c_int]
        L.mscnn_conv2d_plan_plane_columns.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.mscnn_debug_wgemm_schedule.restype = C.c_long
        L.mscnn_debug_wgemm_schedule.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long, C.c_void_p]
        L.mscnn_debug_conv_plan_class.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.mscnn_conv2d_plan_stage_ms.argtypes = [C.c_void_p, C.c_void_p]
        for f in ("mscnn_conv2d_packed_weight_bytes", "mscnn_conv2d_workspace_bytes"):
            getattr(L, f).restype = C.c_size_t
            getattr(L, f).argtypes = [C.c_void_p]
        L.mscnn_conv2d_plan_destroy.argtypes = [C.c_void_p]
        L.mscnn_conv2d_plan_destroy.restype = None
        L.mscnn_conv2d_plan_set_batch.argtypes = [C.c_void_p, C.c_int]
        L.mscnn_conv2d_pack_weights.argtypes = [C.c_void_p] * 4
        L.mscnn_conv2d_fwd_f32.argtypes = [C.c_void_p] * 7 + [C.c_size_t, C.c_void_p]
        L.mscnn_conv2d_fwd_pool_f32.argtypes = [C.c_void_p] * 8 + [C.c_size_t, C.c_void_p]
        L.mscnn_conv2d_plan_can_pool.argtypes = [C.c_void_p]
        L.mscnn_conv2d_plan_can_fuse_roipool.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.mscnn_conv2d_plan_can_chain.argtypes = [C.c_void_p, C.c_void_p]
        L.mscnn_conv2d_plan_can_pool_only.argtypes = [C.c_void_p]
        L.mscnn_conv2d_fwd_chain_f32.argtypes = [C.c_void_p] * 8 + [C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
        L.mscnn_conv2d_roipool_workspace_bytes.restype = C.c_size_t
        L.mscnn_conv2d_roipool_workspace_bytes.argtypes = [C.c_void_p] + [C.c_int] * 4
        L.mscnn_conv2d_fwd_roipool_pair_f32.argtypes = ([C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_float, C.c_float, C.c_float]
                                                        + [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p])
        L.mscnn_roipool_maps_bytes.restype = C.c_size_t
        L.mscnn_roipool_maps_bytes.argtypes = [C.c_int] * 4
        L.mscnn_roipool_maps_build_f32.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p]
        L.mscnn_conv2d_plan_weight_layout.argtypes = [C.c_void_p]
        L.mscnn_conv2d_plan_weight_layout.restype = C.c_ulonglong
        L.mscnn_relu_fwd_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p]
        L.mscnn_pool_out_dims.argtypes = [C.c_int] * 8 + [C.c_void_p, C.c_void_p]
        L.mscnn_pool2d_fwd_f32.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 11 + [C.c_void_p]
        L.mscnn_inner_product_fwd_f32.argtypes = [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p]
        L.mscnn_concat_channels_f32.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]
        L.mscnn_deconv_depthwise_fwd_f32.argtypes = [C.c_void_p] * 4 + [C.c_int] * 10 + [C.c_void_p]
        L.mscnn_deconv2d_fwd_f32.argtypes = [C.c_void_p] * 4 + [C.c_int] * 12 + [C.c_void_p]
        L.mscnn_softmax_fwd_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.mscnn_roipool_fwd_f32.argtypes = ([C.c_void_p] * 3 + [C.c_int] * 7 + [C.c_float, C.c_float] + [C.c_int] * 2
                                            + [C.c_void_p])
        L.mscnn_roipool_pair_fwd_f32.argtypes = ([C.c_void_p] * 3 + [C.c_int] * 7 + [C.c_float, C.c_float, C.c_int, C.c_float, C.c_int, C.c_int]
                                                 + [C.c_void_p])
        L.mscnn_roialign_fwd_f32.argtypes = [C.c_void_p] * 3 + [C.c_int] * 7 + [C.c_float, C.c_float, C.c_void_p]
        L.mscnn_roialign_ave_fwd_f32.argtypes = ([C.c_void_p] * 3 + [C.c_int] * 7 + [C.c_float, C.c_float] + [C.c_int] * 2
                                                 + [C.c_void_p])
        L.mscnn_roialign_ave_pair_fwd_f32.argtypes = ([C.c_void_p] * 3 + [C.c_int] * 7
                                                      + [C.c_float, C.c_float, C.c_int, C.c_float, C.c_int, C.c_int] + [C.c_void_p])
        L.mscnn_eltwise_fwd_f32.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        L.mscnn_boxoutput_workspace_bytes.restype = C.c_size_t
        L.mscnn_boxoutput_workspace_bytes.argtypes = [C.c_void_p]
        L.mscnn_boxoutput_max_rows.argtypes = [C.c_void_p]
        L.mscnn_boxoutput_fwd_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                              C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.mscnn_boxoutput_batch_workspace_bytes.restype = C.c_size_t
        L.mscnn_boxoutput_batch_workspace_bytes.argtypes = [C.c_void_p]
        L.mscnn_boxoutput_batch_fwd_f32.argtypes = L.mscnn_boxoutput_fwd_f32.argtypes
        L.mscnn_nms_workspace_bytes.restype = C.c_size_t
        L.mscnn_nms_workspace_bytes.argtypes = [C.c_int]
        L.mscnn_nms_greedy_f32.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                           C.c_void_p]
        L.mscnn_decodebbox_fwd_f32.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mscnn_detections_workspace_bytes.restype = C.c_size_t
        L.mscnn_detections_workspace_bytes.argtypes = [C.c_int]
        L.mscnn_detections_fwd.argtypes = [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]
        L.mscnn_detections_multi_pack_bytes.restype = C.c_size_t
        L.mscnn_detections_multi_pack_bytes.argtypes = [C.c_int, C.c_int]
        L.mscnn_detections_multi_workspace_bytes.restype = C.c_size_t
        L.mscnn_detections_multi_workspace_bytes.argtypes = [C.c_int, C.c_int]
        L.mscnn_detections_multi_fwd.argtypes = ([C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                 C.c_void_p, C.c_size_t, C.c_void_p])
        L.mscnn_detections_cascade_multi_workspace_bytes.restype = C.c_size_t
        L.mscnn_detections_cascade_multi_workspace_bytes.argtypes = [C.c_int, C.c_int]
        L.mscnn_detections_cascade_multi_fwd.argtypes = ([C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                         C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p])
        L.mscnn_nms_params_resolve.argtypes = [C.c_void_p, C.c_void_p]
        L.mscnn_nms_params_from_names.argtypes = [C.c_char_p, C.c_char_p, C.c_double, C.c_double, C.c_float, C.c_void_p]
        L.mscnn_detections_nms_fwd.argtypes = [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]
        L.mscnn_detections_cascade_nms_fwd.argtypes = ([C.c_void_p, C.c_float] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 4 +
                                                       [C.c_size_t, C.c_void_p])
        L.mscnn_detections_multi_nms_fwd.argtypes = ([C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 3 +
                                                     [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p])
        L.mscnn_detections_cascade_multi_nms_fwd.argtypes = ([C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                              C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p])
        L.mscnn_detections_candidates_bytes.restype = C.c_size_t
        L.mscnn_detections_candidates_bytes.argtypes = [C.c_int, C.c_int]
        L.mscnn_detections_candidates_reset.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.mscnn_detections_candidates_add.argtypes = ([C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p] * 3 +
                                                      [C.c_int, C.c_void_p, C.c_int, C.c_void_p])
        L.mscnn_detections_candidates_cascade_add.argtypes = ([C.c_void_p, C.c_void_p, C.c_float, C.c_void_p] + [C.c_int] * 4 +
                                                              [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p])
        L.mscnn_detections_candidates_add_views.argtypes = ([C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p] * 3 +
                                                            [C.c_int, C.c_void_p, C.c_int, C.c_void_p])
        L.mscnn_detections_candidates_cascade_add_views.argtypes = ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p] + [C.c_int] * 5 +
                                                                    [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p])
        L.mscnn_preprocess_views_workspace_bytes.restype = C.c_size_t
        L.mscnn_preprocess_views_workspace_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.mscnn_preprocess_views_u8_f32.argtypes = ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                     C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p])
        L.mscnn_detections_merge_workspace_bytes.restype = C.c_size_t
        L.mscnn_detections_merge_workspace_bytes.argtypes = [C.c_int, C.c_int]
        L.mscnn_detections_merge_fwd.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                                 C.c_void_p]
        L.mscnn_detections_merge_vote_fwd.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.mscnn_detections_merge_soft_workspace_bytes.restype = C.c_size_t
        L.mscnn_detections_merge_soft_workspace_bytes.argtypes = [C.c_int, C.c_int]
        L.mscnn_detections_merge_soft_fwd.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                                      C.c_void_p]
        L.mscnn_detections_merge_matrix_workspace_bytes.restype = C.c_size_t
        L.mscnn_detections_merge_matrix_workspace_bytes.argtypes = [C.c_int, C.c_int]
        L.mscnn_detections_merge_matrix_fwd.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.mscnn_detections_merge_wbf_workspace_bytes.restype = C.c_size_t
        L.mscnn_detections_merge_wbf_workspace_bytes.argtypes = [C.c_int, C.c_int]
        L.mscnn_detections_merge_wbf_fwd.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_size_t, C.c_void_p]
        L.mscnn_detections_merge_seq_workspace_bytes.restype = C.c_size_t
        L.mscnn_detections_merge_seq_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
        L.mscnn_detections_merge_seq_fwd.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_size_t, C.c_void_p]
        L.mscnn_tracks_state_bytes.restype = C.c_size_t
        L.mscnn_tracks_state_bytes.argtypes = [C.c_int, C.c_int]
        L.mscnn_tracks_state_reset.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.mscnn_tracks_update_fwd.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                              C.c_void_p]
        L.mscnn_tracks_state_reset_slots.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.mscnn_tracks_update_streams_fwd.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                      C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.mscnn_tracks_kalman_state_bytes.restype = C.c_size_t
        L.mscnn_tracks_kalman_state_bytes.argtypes = [C.c_int, C.c_int]
        L.mscnn_tracks_update_kalman_fwd.argtypes = [C.c_void_p]
        L.mscnn_tracks_update_assign_fwd.argtypes = [C.c_void_p]
        L.mscnn_render_detections_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                 C.c_void_p, C.c_void_p]
        L.mscnn_render_glyph_rows.argtypes = [C.c_int, C.c_void_p]
        L.mscnn_proposals_multi_pack_bytes.restype = C.c_size_t
        L.mscnn_proposals_multi_pack_bytes.argtypes = [C.c_int, C.c_int]
        L.mscnn_proposals_multi_fwd.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.mscnn_rois_reason_text.restype = C.c_char_p
        L.mscnn_rois_reason_text.argtypes = [C.c_int]
        L.mscnn_rois_ingest_f32.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 7
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise MscnnError(f"mscnn status {rc}: {lib().mscnn_last_error().decode()}")


def _dev(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise MscnnError("libmscnn_hip has no CPU path: tensor must live on the GPU")
    if not t.is_contiguous():
        raise MscnnError("tensor must be contiguous")
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class ConvPlan:
    """Owns a mscnn_conv_plan plus its packed weights and stream-K workspace (device memory)."""

    def __init__(self, N, Cin, H, W, Cout, Kh, Kw, pad=(0, 0), stride=(1, 1), group=1, relu=False, device="cuda",
                 algo=ALGO_AUTO, tune_variant=0, tune_grid=0, tune_flags=0):
        self.desc = ConvDesc(N, Cin, H, W, Cout, Kh, Kw, pad[0], pad[1], stride[0], stride[1], group, int(relu),
                             algo, tune_variant, tune_grid, tune_flags)
        self._p = C.c_void_p()
        _check(lib().mscnn_conv2d_plan_create(C.byref(self.desc), C.byref(self._p)))
        self.device = device
        self.packed = None
        self.ws = None
        self.w = None
        self._alloc()

    def _alloc(self):
        pb = lib().mscnn_conv2d_packed_weight_bytes(self._p)
        wb = lib().mscnn_conv2d_workspace_bytes(self._p)
        if pb and (self.packed is None or self.packed.numel() * 4 < pb):
            self.packed = torch.empty(pb // 4, dtype=torch.float32, device=self.device)
        if wb and (self.ws is None or self.ws.numel() * 4 < wb):
            self.ws = torch.empty(wb // 4, dtype=torch.float32, device=self.device)

    @property
    def kernel(self):
        return lib().mscnn_conv2d_plan_kernel(self._p).decode()

    @property
    def dtype(self):
        return lib().mscnn_conv2d_plan_dtype(self._p).decode()

    @property
    def flops(self):
        return lib().mscnn_conv2d_plan_flops(self._p)

    @property
    def executed_flops(self):
        return lib().mscnn_conv2d_plan_executed_flops(self._p)

    def plane_columns(self):
        """Live GEMM columns of each transform plane (mscnn_conv2d_plan_plane_columns); [] for a plan that is not Winograd."""
        out = (C.c_int * 36)()
        n = lib().mscnn_conv2d_plan_plane_columns(self._p, out, 36)
        return [int(out[i]) for i in range(n)]

    def debug_wgemm_schedule(self, whole_tiles=False):
        """Host replay of the plane GEMM's schedule (mscnn_debug_wgemm_schedule): (info dict, rows [n][7] as a numpy array of
        {slot, plane, column tile, row tile, k0, k1, part}), or None where the plan has no wgemm GEMM."""
        import numpy as np
        info = (C.c_int * 8)()
        n = lib().mscnn_debug_wgemm_schedule(self._p, int(bool(whole_tiles)), None, 0, info)
        if n < 0:
            return None
        rows = np.zeros((max(n, 1), 7), dtype=np.int32)
        got = lib().mscnn_debug_wgemm_schedule(self._p, int(bool(whole_tiles)), rows.ctypes.data_as(C.c_void_p), n, info)
        assert got == n
        keys = ("tiles", "MT", "KI", "G", "full_q", "planes", "BN", "ragged")
        return {k: int(info[i]) for i, k in enumerate(keys)}, rows[:n]

    def plan_class(self):
        """The plan's discrete decisions (mscnn_debug_conv_plan_class) as a dict field name -> int, in the library's field order."""
        names = C.c_char_p()
        n = lib().mscnn_debug_conv_plan_class(self._p, None, 0, C.byref(names))
        out = (C.c_int * n)()
        assert lib().mscnn_debug_conv_plan_class(self._p, out, n, None) == n
        fields = names.value.decode().split(",")
        assert len(fields) == n
        return {f: int(out[i]) for i, f in enumerate(fields)}

    def set_profiling(self, on=True):
        _check(lib().mscnn_conv2d_plan_set_profiling(self._p, int(on)))

    def stage_ms(self):
        """(input transform, MFMA GEMM kernels, output transform) of the last forward, HIP events on its stream."""
        out = (C.c_float * 3)()
        _check(lib().mscnn_conv2d_plan_stage_ms(self._p, out))
        return tuple(out)

    def out_shape(self):
        d = self.desc
        return (d.N, d.Cout, (d.H + 2 * d.pad_h - d.Kh) // d.stride_h + 1, (d.W + 2 * d.pad_w - d.Kw) // d.stride_w + 1)

    def set_batch(self, N):
        before, had = lib().mscnn_conv2d_plan_weight_layout(self._p), self.packed
        _check(lib().mscnn_conv2d_plan_set_batch(self._p, N))
        self.desc.N = N
        self._alloc()
        if getattr(self, "w", None) is not None and self.packed is not None and \
                (lib().mscnn_conv2d_plan_weight_layout(self._p) != before or self.packed is not had):
            self.pack(self.w)      # another kernel family (or a new buffer): the packed weights must be rebuilt

    def pack(self, w):
        self.w = w
        if self.packed is not None:
            _check(lib().mscnn_conv2d_pack_weights(self._p, _dev(w), _dev(self.packed), _stream()))

    @property
    def publishes_amax(self):
        return bool(lib().mscnn_conv2d_plan_publishes_amax(self._p))

    def set_amax_io(self, in_bound=None, out_amax=None):
        """max |x| hand-over (mscnn_conv2d_plan_set_amax_io): int32 device tensors of AMAX_SLOTS float bit patterns."""
        self._amax = (in_bound, out_amax)      # keep them alive
        _check(lib().mscnn_conv2d_plan_set_amax_io(self._p, _dev(in_bound), _dev(out_amax)))

    @property
    def can_pool(self):
        return bool(lib().mscnn_conv2d_plan_can_pool(self._p))

    def forward(self, x, bias=None, out=None, pool_out=None):
        """pool_out: tensor [N, Cout, ceil(Ho/2), ceil(Wo/2)] that receives the fused MAX 2x2 / stride 2 pooling."""
        if out is None:
            out = torch.empty(self.out_shape(), dtype=torch.float32, device=x.device)
        wsb = self.ws.numel() * 4 if self.ws is not None else 0
        _check(lib().mscnn_conv2d_fwd_pool_f32(self._p, _dev(x), _dev(self.w), _dev(self.packed), _dev(bias), _dev(out),
                                               _dev(pool_out), _dev(self.ws), wsb, _stream()))
        return out

    @property
    def can_pool_only(self):
        return bool(lib().mscnn_conv2d_plan_can_pool_only(self._p))

    def can_chain(self, nxt):
        return bool(lib().mscnn_conv2d_plan_can_chain(self._p, nxt._p))

    def forward_chain(self, x, nxt, bias=None, out=None, pool_out=None, write_y=True):
        """mscnn_conv2d_fwd_chain_f32: x None = this plan's planes were prepared (it was the `nxt` of the previous call);
        nxt given = its planes are written by this plan's output stage (y only if write_y); nxt None = ordinary output."""
        if out is None and write_y:
            out = torch.empty(self.out_shape(), dtype=torch.float32, device=self.ws.device)
        wsb = self.ws.numel() * 4
        _check(lib().mscnn_conv2d_fwd_chain_f32(self._p, nxt._p if nxt is not None else None, _dev(x), _dev(self.packed), _dev(bias),
                                                _dev(out) if write_y else None, _dev(pool_out), _dev(self.ws), wsb,
                                                _dev(nxt.ws) if nxt is not None else None, nxt.ws.numel() * 4 if nxt is not None else 0,
                                                _stream()))
        return out

    def can_fuse_roipool(self, Cc, pooled_h, pooled_w):
        return bool(lib().mscnn_conv2d_plan_can_fuse_roipool(self._p, Cc, pooled_h, pooled_w))

    def forward_roipool_pair(self, feat, rois, spatial_scale, pad_a, pad_b, bias=None, out=None, maps=None):
        """ROIPooling x 2 (pad_a -> channels [0, C), pad_b -> [C, 2C)) fused into this convolution's Winograd input stage
        (mscnn_conv2d_fwd_roipool_pair_f32): y = conv(concat(roipool(feat, pad_a), roipool(feat, pad_b)))."""
        N, Cc, H, W = feat.shape
        need = lib().mscnn_conv2d_roipool_workspace_bytes(self._p, N, Cc, H, W)
        if self.ws is None or self.ws.numel() * 4 < need:
            self.ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=feat.device)
        if out is None:
            out = torch.empty(self.out_shape(), dtype=torch.float32, device=feat.device)
        _check(lib().mscnn_conv2d_fwd_roipool_pair_f32(self._p, _dev(feat), _dev(maps), N, Cc, H, W, _dev(rois), spatial_scale, pad_a, pad_b,
                                                       _dev(self.packed), _dev(bias), _dev(out), _dev(self.ws), self.ws.numel() * 4,
                                                       _stream()))
        return out

    def __del__(self):
        try:
            if self._p:
                lib().mscnn_conv2d_plan_destroy(self._p)
                self._p = None
        except Exception:
            pass


def conv2d(x, w, bias=None, pad=(0, 0), stride=(1, 1), group=1, relu=False, algo=ALGO_AUTO):
    N, Cin, H, W = x.shape
    Cout, _, Kh, Kw = w.shape
    plan = ConvPlan(N, Cin, H, W, Cout, Kh, Kw, pad, stride, group, relu, device=x.device, algo=algo)
    plan.pack(w)
    y = plan.forward(x, bias)
    torch.cuda.current_stream().synchronize()   # plan buffers die with the plan
    return y


def relu(x, slope=0.0, inplace=False):
    y = x if inplace else torch.empty_like(x)
    _check(lib().mscnn_relu_fwd_f32(_dev(x), _dev(y), x.numel(), slope, _stream()))
    return y


def sum_squares(x):
    """mscnn_sum_squares_f32: a float64 device scalar holding sum x^2."""
    out = torch.zeros(1, dtype=torch.float64, device=x.device)
    _check(lib().mscnn_sum_squares_f32(_dev(x), x.numel(), _dev(out), _stream()))
    return out


def max_rel_diff(a, ref, floor=1.0):
    """mscnn_max_rel_diff_f32: max |a - ref| / max(floor, |ref|) (+inf when a NaN is involved), a float32 device scalar."""
    out = torch.zeros(1, dtype=torch.float32, device=a.device)
    _check(lib().mscnn_max_rel_diff_f32(_dev(a), _dev(ref), a.numel(), floor, _dev(out), _stream()))
    return out


def max_rel_diff_strided(a, a_stride, ref, ref_stride, planes, run, sumsq, sumsq_count):
    """mscnn_max_rel_diff_strided_f32: the same over `planes` runs of `run` floats (plane p at a + p * a_stride / ref + p * ref_stride),
    floor = max(1, sqrt(sumsq[0] / sumsq_count)) read on the device from `sumsq` (a float64 device scalar)."""
    out = torch.zeros(1, dtype=torch.float32, device=a.device)
    _check(lib().mscnn_max_rel_diff_strided_f32(_dev(a), a_stride, _dev(ref), ref_stride, planes, run, _dev(sumsq), float(sumsq_count), _dev(out),
                                                _stream()))
    return out


def store_words(dst, values):
    """mscnn_store_words_i32: dst[0 .. len(values)) = values (1 .. 4 int32 words) in one launch."""
    arr = (C.c_int * len(values))(*[int(v) for v in values])
    _check(lib().mscnn_store_words_i32(_dev(dst), arr, len(values), _stream()))


def pool_out_dim(i, k, p, s):
    return lib().mscnn_pool_out_dim(i, k, p, s)


def pool_out_dims(H, W, kernel, pad, stride):
    """(Ho, Wo) by mscnn_pool_out_dims, the one owner of the pooling output shape; MscnnError for what the reference's set-up refuses."""
    ho, wo = C.c_int(), C.c_int()
    _check(lib().mscnn_pool_out_dims(H, W, kernel[0], kernel[1], pad[0], pad[1], stride[0], stride[1], C.byref(ho), C.byref(wo)))
    return ho.value, wo.value


def pool2d(x, kernel=(2, 2), pad=(0, 0), stride=(2, 2), method="MAX"):
    N, Cc, H, W = x.shape
    Ho, Wo = pool_out_dims(H, W, kernel, pad, stride)
    y = torch.empty((N, Cc, Ho, Wo), dtype=torch.float32, device=x.device)
    _check(lib().mscnn_pool2d_fwd_f32(_dev(x), _dev(y), N, Cc, H, W, kernel[0], kernel[1], pad[0], pad[1],
                                      stride[0], stride[1], 0 if method == "MAX" else 1, _stream()))
    return y


def inner_product_wg_supported(M, N, K):
    return bool(lib().mscnn_inner_product_wg_supported(M, N, K))


def inner_product_wg(x, w, bias=None, relu=False, wt=None, out=None):
    """InnerProduct on the plane-GEMM kernel (mscnn_inner_product_wg_*); wt: the transposed weights from a previous call (returned)."""
    M = x.shape[0]
    K = x.numel() // M
    Nn = w.shape[0]
    if wt is None:
        wt = torch.empty((K, Nn), dtype=torch.float32, device=x.device)
        _check(lib().mscnn_inner_product_wg_pack(_dev(w), _dev(wt), Nn, K, _stream()))
    wb = lib().mscnn_inner_product_wg_workspace_bytes(M, Nn, K)
    ws = torch.empty((wb + 3) // 4, dtype=torch.float32, device=x.device)
    y = out if out is not None else torch.empty((M, Nn), dtype=torch.float32, device=x.device)
    _check(lib().mscnn_inner_product_wg_fwd(_dev(x), _dev(wt), _dev(bias), _dev(y), M, Nn, K, int(relu), _dev(ws), wb, _stream()))
    torch.cuda.current_stream().synchronize()
    return y, wt


def inner_product(x, w, bias=None, relu=False):
    M = x.shape[0]
    K = x.numel() // max(M, 1) if M else w.shape[1]
    Nn = w.shape[0]
    y = torch.empty((M, Nn), dtype=torch.float32, device=x.device)
    _check(lib().mscnn_inner_product_fwd_f32(_dev(x), _dev(w), _dev(bias), _dev(y), M, Nn, K, int(relu), _stream()))
    return y


def inner_product_x3(x, w, bias=None, relu=False, packed=None):
    """Split-fp16 InnerProduct (fp32-grade): w [N][K] is packed into exactly split fp16 hi + lo units, x is split on the device
    with a scale from its measured max |x|; three fp16 MFMAs per operand pair, fp32 accumulate."""
    M, K = x.shape[0], int(x.numel() // max(x.shape[0], 1))
    Nn = w.shape[0]
    if not lib().mscnn_inner_product_x3_supported(Nn, K):
        raise MscnnError(f"inner_product x3 needs N >= 128 and K % 32 == 0 (N={Nn}, K={K})")
    if packed is None:
        packed = torch.empty(lib().mscnn_inner_product_x3_packed_bytes(Nn, K), dtype=torch.uint8, device=x.device)
        _check(lib().mscnn_inner_product_x3_pack(_dev(w), _dev(packed), Nn, K, _stream()))
    wb = lib().mscnn_inner_product_x3_workspace_bytes(M, Nn, K)
    ws = torch.empty(wb, dtype=torch.uint8, device=x.device)
    y = torch.empty((M, Nn), dtype=torch.float32, device=x.device)
    _check(lib().mscnn_inner_product_x3_fwd(_dev(x), _dev(packed), _dev(bias), _dev(y), M, Nn, K, int(relu), None, _dev(ws), wb, _stream()))
    return y


def inner_product_f16(x, w, bias=None, relu=False):
    """fp16-operand InnerProduct: w is converted once to fp16 (here per call), x on the fly, fp32 accumulate."""
    M = x.shape[0]
    Nn, K = w.shape[0], w[0].numel()
    if not lib().mscnn_inner_product_f16_supported(Nn, K):
        raise MscnnError(f"inner_product f16 needs N >= 64 and K % 8 == 0 (N={Nn}, K={K})")
    w16 = torch.empty(Nn * K, dtype=torch.float16, device=x.device)
    _check(lib().mscnn_inner_product_pack_f16(_dev(w), _dev(w16), Nn, K, _stream()))
    y = torch.empty((M, Nn), dtype=torch.float32, device=x.device)
    _check(lib().mscnn_inner_product_fwd_f16(_dev(x), _dev(w16), _dev(bias), _dev(y), M, Nn, K, int(relu), _stream()))
    return y


def concat_channels(xs):
    N = xs[0].shape[0]
    inner = xs[0][0, 0].numel()
    ctot = sum(t.shape[1] for t in xs)
    y = torch.empty((N, ctot) + tuple(xs[0].shape[2:]), dtype=torch.float32, device=xs[0].device)
    off = 0
    for t in xs:
        _check(lib().mscnn_concat_channels_f32(_dev(t), _dev(y), N, t.shape[1], inner, ctot, off, _stream()))
        off += t.shape[1]
    return y


def deconv_depthwise(x, w, bias=None, pad=(0, 0), stride=(1, 1)):
    N, Cc, H, W = x.shape
    Kh, Kw = w.shape[2], w.shape[3]
    Ho, Wo = stride[0] * (H - 1) + Kh - 2 * pad[0], stride[1] * (W - 1) + Kw - 2 * pad[1]
    y = torch.empty((N, Cc, Ho, Wo), dtype=torch.float32, device=x.device)
    _check(lib().mscnn_deconv_depthwise_fwd_f32(_dev(x), _dev(w), _dev(bias), _dev(y), N, Cc, H, W, Kh, Kw,
                                                pad[0], pad[1], stride[0], stride[1], _stream()))
    return y


def deconv2d(x, w, bias=None, pad=(0, 0), stride=(1, 1), group=1):
    """mscnn_deconv2d_fwd_f32: transposed convolution with any group / kernel / stride / pad, w [Cin][Cout / group][Kh][Kw]
    (group == Cin == Cout goes to the depthwise kernels inside the op)."""
    N, Cin, H, W = x.shape
    Kh, Kw = w.shape[2], w.shape[3]
    Cout = w.shape[1] * group
    Ho, Wo = stride[0] * (H - 1) + Kh - 2 * pad[0], stride[1] * (W - 1) + Kw - 2 * pad[1]
    y = torch.empty((N, Cout, Ho, Wo), dtype=torch.float32, device=x.device)
    _check(lib().mscnn_deconv2d_fwd_f32(_dev(x), _dev(w), _dev(bias), _dev(y), N, Cin, H, W, Cout, Kh, Kw, pad[0], pad[1],
                                        stride[0], stride[1], group, _stream()))
    return y


def softmax(x, axis=1):
    outer = 1
    for d in x.shape[:axis]:
        outer *= d
    inner = 1
    for d in x.shape[axis + 1:]:
        inner *= d
    y = torch.empty_like(x)
    _check(lib().mscnn_softmax_fwd_f32(_dev(x), _dev(y), outer, x.shape[axis], inner, _stream()))
    return y


def roipool(feat, rois, pooled_h, pooled_w, spatial_scale, pad_ratio=0.0, out=None, c_total=None, c_offset=0):
    N, Cc, H, W = feat.shape
    R = rois.shape[0]
    c_total = c_total or Cc
    if out is None:
        out = torch.empty((R, c_total, pooled_h, pooled_w), dtype=torch.float32, device=feat.device)
    _check(lib().mscnn_roipool_fwd_f32(_dev(feat), _dev(rois), _dev(out), R, N, Cc, H, W, pooled_h, pooled_w,
                                       spatial_scale, pad_ratio, c_total, c_offset, _stream()))
    return out


def roipool_maps(feat, stream=None):
    """The four maps the fused ROI-pooling stage reads (mscnn_roipool_maps_build_f32), built on `stream` (default: the current one)."""
    N, Cc, H, W = feat.shape
    maps = torch.empty(lib().mscnn_roipool_maps_bytes(N, Cc, H, W) // 4, dtype=torch.float32, device=feat.device)
    _check(lib().mscnn_roipool_maps_build_f32(_dev(feat), _dev(maps), N, Cc, H, W, C.c_void_p(stream.cuda_stream) if stream is not None else _stream()))
    return maps


def roipool_pair(feat, rois, pooled_h, pooled_w, spatial_scale, pad_a, pad_b):
    """Two ROI poolings (context paddings pad_a / pad_b) into channels [0, C) and [C, 2C) of one output, one launch."""
    N, Cc, H, W = feat.shape
    R = rois.shape[0]
    out = torch.empty((R, 2 * Cc, pooled_h, pooled_w), dtype=torch.float32, device=feat.device)
    _check(lib().mscnn_roipool_pair_fwd_f32(_dev(feat), _dev(rois), _dev(out), R, N, Cc, H, W, pooled_h, pooled_w, spatial_scale,
                                            pad_a, 0, pad_b, Cc, 2 * Cc, _stream()))
    return out


def roialign(feat, rois, pooled_h, pooled_w, spatial_scale, pad_ratio=0.0):
    N, Cc, H, W = feat.shape
    R = rois.shape[0]
    out = torch.empty((R, Cc, pooled_h + 1, pooled_w + 1), dtype=torch.float32, device=feat.device)
    _check(lib().mscnn_roialign_fwd_f32(_dev(feat), _dev(rois), _dev(out), R, N, Cc, H, W, pooled_h, pooled_w, spatial_scale,
                                        pad_ratio, _stream()))
    return out


def roialign_ave(feat, rois, ph, pw, scale, pad, out=None, c_total=None, c_offset=0):
    """ROIAlign + the 2x2 / stride 1 AVE pooling in one launch, into channels [c_offset, c_offset + C) of out[R][c_total][ph][pw]."""
    N, Cc, H, W = feat.shape
    R = rois.shape[0]
    c_total = c_total or Cc
    if out is None:
        out = torch.empty((R, c_total, ph, pw), dtype=torch.float32, device=feat.device)
    _check(lib().mscnn_roialign_ave_fwd_f32(_dev(feat), _dev(rois), _dev(out), R, N, Cc, H, W, ph, pw, scale, pad, c_total, c_offset,
                                            _stream()))
    return out


def roialign_ave_pair(feat, rois, ph, pw, scale, pad_a, pad_b, out=None, c_total=None, c_offset_a=0, c_offset_b=None):
    """The ROIAlign head in one launch: both context windows, the 2x2 AVE pooling and the Concat (pad_a -> channels
    [c_offset_a, + C), pad_b -> [c_offset_b, + C); c_offset_b defaults to the window behind a's)."""
    N, Cc, H, W = feat.shape
    R = rois.shape[0]
    if c_offset_b is None:
        c_offset_b = c_offset_a + Cc
    c_total = c_total or max(c_offset_a, c_offset_b) + Cc
    if out is None:
        out = torch.empty((R, c_total, ph, pw), dtype=torch.float32, device=feat.device)
    _check(lib().mscnn_roialign_ave_pair_fwd_f32(_dev(feat), _dev(rois), _dev(out), R, N, Cc, H, W, ph, pw, scale, pad_a, c_offset_a,
                                                 pad_b, c_offset_b, c_total, _stream()))
    return out


def eltwise(xs, op="SUM", coeffs=None):
    n = len(xs)
    for t in xs:
        _dev(t)
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in xs])
    cf = (C.c_float * n)(*coeffs) if coeffs is not None and len(coeffs) else None
    y = torch.empty_like(xs[0])
    _check(lib().mscnn_eltwise_fwd_f32(ptrs, n, cf, _dev(y), y.numel(), {"PROD": 0, "SUM": 1, "MAX": 2}[op], _stream()))
    return y


def make_boxoutput_desc(head_shapes, num, channels, field_w, field_h, downsample, fg_thr=-5.0, iou_thr=0.65,
                        nms_type="IOU", field_whr=2.0, field_xyr=2.0, max_nms_num=2000, max_post_nms_num=0,
                        min_size=15.0, bbox_mean=None, bbox_std=None):
    d = BoxOutputDesc()
    d.num_heads = len(head_shapes); d.num = num; d.channels = channels
    for j, (h, w) in enumerate(head_shapes):
        d.head_h[j] = h; d.head_w[j] = w
        d.field_w[j] = field_w[j]; d.field_h[j] = field_h[j]; d.downsample_rate[j] = downsample[j]
    d.fg_thr = fg_thr; d.iou_thr = iou_thr; d.nms_mode = NMS_MODES[nms_type]
    d.field_whr = field_whr; d.field_xyr = field_xyr
    d.max_nms_num = max_nms_num; d.max_post_nms_num = max_post_nms_num; d.min_size = min_size
    if bbox_mean is not None and bbox_std is not None and len(bbox_mean) and len(bbox_std):
        d.do_bbox_norm = 1
        for k in range(4):
            d.bbox_mean[k] = bbox_mean[k]; d.bbox_std[k] = bbox_std[k]
    return d


class BoxOutput:
    """Device-resident BoxOutput layer state: descriptor + workspace + output buffers.  one_pass: every image of the batch side
    by side (mscnn_boxoutput_batch_fwd_f32) instead of image after image -- the same words either way."""

    def __init__(self, desc, device="cuda", one_pass=False):
        self.desc = desc
        L = lib()
        self._fwd = L.mscnn_boxoutput_batch_fwd_f32 if one_pass else L.mscnn_boxoutput_fwd_f32
        wb = (L.mscnn_boxoutput_batch_workspace_bytes if one_pass else L.mscnn_boxoutput_workspace_bytes)(C.byref(desc))
        if wb == 0:
            raise MscnnError(lib().mscnn_last_error().decode())
        self.cap = lib().mscnn_boxoutput_max_rows(C.byref(desc))
        self.ws = torch.empty(wb, dtype=torch.uint8, device=device)
        self.rois = torch.empty((self.cap, 5), dtype=torch.float32, device=device)
        self.props = torch.empty((self.cap, 6), dtype=torch.float32, device=device)
        self.aids = torch.empty(self.cap, dtype=torch.int32, device=device)
        self.count = torch.zeros(2, dtype=torch.int32, device=device)

    def forward_async(self, heads):
        n = self.desc.num_heads
        ptrs = (C.c_void_p * n)(*[h.data_ptr() for h in heads])
        for h in heads:
            _dev(h)
        _check(self._fwd(C.byref(self.desc), ptrs, _dev(self.rois), _dev(self.props), _dev(self.aids),
                         self.cap, _dev(self.count), _dev(self.ws), self.ws.numel(), _stream()))

    def forward(self, heads):
        self.forward_async(heads)
        R, nreal = self.count.tolist()      # the one small D2H of the layer (R drives the next Reshape)
        return self.rois[:R], self.props[:R], self.aids[:R], nreal


_DESC_DEFAULTS = dict(bbox_mean=(0, 0, 0, 0), bbox_std=(0.1, 0.1, 0.2, 0.2), proposal_thr=-10.0, ratios=(1.0, 1.0), org_hw=(375, 1242),
                      nms_overlap=0.5)


def _fill_desc(d, ncls, kw):
    """mscnn_detections_desc d from the keyword arguments of detections() (missing ones: its defaults)."""
    kw = dict(_DESC_DEFAULTS, **kw)
    d.ncls = ncls; d.cls_id = kw["cls_id"]
    for k in range(4):
        d.bbox_mean[k] = kw["bbox_mean"][k]; d.bbox_std[k] = kw["bbox_std"][k]
    d.proposal_thr = kw["proposal_thr"]
    d.ratio_h, d.ratio_w = kw["ratios"]
    d.org_h, d.org_w = kw["org_hw"]
    d.nms_overlap = kw["nms_overlap"]


def detections_cascade(boxes, cls_prob, props, cls_id, det_thr=0.0, ratios=(1.0, 1.0), org_hw=(375, 1242), nms_overlap=0.5, nms=None):
    """Final stage of the cascade drivers (run_cascademscnn.m:84-117) for one cascade stage's blobs.  nms: None (the existing
    entry point), an NmsParams or a dict of nms_params() arguments (mscnn_detections_cascade_nms_fwd)."""
    R = props.shape[0]
    d = DetectionsDesc()      # (of the desc, the cascade stage reads ncls, cls_id, ratio_*, org_* and nms_overlap)
    _fill_desc(d, cls_prob.shape[1], dict(cls_id=cls_id, ratios=ratios, org_hw=org_hw, nms_overlap=nms_overlap))
    dev = props.device
    dets = torch.zeros((max(R, 1), 5), dtype=torch.float64, device=dev)
    ids = torch.zeros(max(R, 1), dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    wb = lib().mscnn_detections_workspace_bytes(R)
    ws = torch.empty(wb, dtype=torch.uint8, device=dev)
    if nms is None:
        _check(lib().mscnn_detections_cascade_fwd(C.byref(d), C.c_float(det_thr), _dev(boxes), _dev(cls_prob), _dev(props), R,
                                                  _dev(dets), _dev(ids), _dev(count), _dev(ws), C.c_size_t(wb), _stream()))
    else:
        _check(lib().mscnn_detections_cascade_nms_fwd(C.byref(d), C.c_float(det_thr), _nms_ref(nms), _dev(boxes), _dev(cls_prob), _dev(props),
                                                      R, _dev(dets), _dev(ids), _dev(count), _dev(ws), C.c_size_t(wb), _stream()))
    D = int(count.item())
    return dets[:D], ids[:D]


def preprocess(img_rgb_u8, out_h, out_w, mean_bgr=(104.0, 117.0, 123.0), out=None):
    """run_mscnn_detection.m:64-69 on the device: uint8 HWC RGB image (cuda tensor) -> the net's (1, 3, out_h, out_w) input."""
    oh, ow, ch = img_rgb_u8.shape
    if ch != 3 or img_rgb_u8.dtype != torch.uint8:
        raise MscnnError("preprocess: expected a uint8 [H, W, 3] image")
    if out is None:
        out = torch.empty((1, 3, out_h, out_w), dtype=torch.float32, device=img_rgb_u8.device)
    L = lib()
    L.mscnn_preprocess_workspace_bytes.restype = C.c_size_t
    wb = L.mscnn_preprocess_workspace_bytes(oh, ow, out_h, out_w)
    ws = torch.empty(wb, dtype=torch.uint8, device=img_rgb_u8.device)
    m = (C.c_float * 3)(*mean_bgr)
    _check(L.mscnn_preprocess_u8_f32(_dev(img_rgb_u8), oh, ow, _dev(out), out_h, out_w, m, _dev(ws), C.c_size_t(wb), _stream()))
    torch.cuda.current_stream().synchronize()     # ws dies with this frame
    return out


def preprocess_batch(frames, out_h, out_w, mean_bgr=(104.0, 117.0, 123.0), out=None):
    """preprocess() for a list of uint8 [h, w, 3] contiguous cuda tensors of their own sizes, in two launches per 32 frames ->
    [B, 3, out_h, out_w]; slice b is bit-identical to preprocess(frames[b], out_h, out_w)."""
    B = len(frames)
    if B < 1:
        raise MscnnError("preprocess_batch: no frames")
    for b, f in enumerate(frames):
        if f.dim() != 3 or f.shape[2] != 3 or f.dtype != torch.uint8 or not f.is_cuda or not f.is_contiguous():
            raise MscnnError(f"preprocess_batch: frame {b} is not a contiguous uint8 [H, W, 3] cuda tensor")
    dev = frames[0].device
    if out is None:
        out = torch.empty((B, 3, out_h, out_w), dtype=torch.float32, device=dev)
    L = lib()
    oh = (C.c_int * B)(*[int(f.shape[0]) for f in frames])
    ow = (C.c_int * B)(*[int(f.shape[1]) for f in frames])
    ptrs = (C.c_void_p * B)(*[f.data_ptr() for f in frames])
    L.mscnn_preprocess_batch_workspace_bytes.restype = C.c_size_t
    L.mscnn_preprocess_batch_workspace_bytes.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    wb = L.mscnn_preprocess_batch_workspace_bytes(B, oh, ow, out_h, out_w)
    ws = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
    m = (C.c_float * 3)(*mean_bgr)
    _check(L.mscnn_preprocess_batch_u8_f32(ptrs, oh, ow, B, _dev(out), out_h, out_w, m, _dev(ws), C.c_size_t(wb), _stream()))
    torch.cuda.current_stream().synchronize()     # ws dies with this batch
    return out


class PreprocessView(C.Structure):
    """mscnn_preprocess_view: window [y0, y0 + h) x [x0, x0 + w) of frame `frame`, reversed along x when flip_x."""
    _fields_ = [("frame", C.c_int), ("x0", C.c_int), ("y0", C.c_int), ("w", C.c_int), ("h", C.c_int), ("flip_x", C.c_int)]


def view_array(views):
    """views: dicts with frame (0), x0, y0, w, h, flip_x (0) -> the PreprocessView array."""
    arr = (PreprocessView * max(len(views), 1))()
    for i, v in enumerate(views):
        arr[i].frame, arr[i].x0, arr[i].y0, arr[i].w, arr[i].h = int(v.get("frame", 0)), int(v["x0"]), int(v["y0"]), int(v["w"]), int(v["h"])
        arr[i].flip_x = int(v.get("flip_x", 0))
    return arr


def preprocess_views(frames, views, out_h, out_w, mean_bgr=(104.0, 117.0, 123.0), out=None, ws=None):
    """mscnn_preprocess_views_u8_f32: frames is a list of contiguous uint8 [h, w, 3] cuda tensors, views a list of dicts (frame, x0,
    y0, w, h, flip_x) -> [len(views), 3, out_h, out_w]; slice v is bit-identical to preprocess() of a contiguous copy of the window
    (mirrored when flip_x).  Two launches per 32 views; no copy of a window is made."""
    F, V = len(frames), len(views)
    for b, f in enumerate(frames):
        if f.dim() != 3 or f.shape[2] != 3 or f.dtype != torch.uint8 or not f.is_cuda or not f.is_contiguous():
            raise MscnnError(f"preprocess_views: frame {b} is not a contiguous uint8 [H, W, 3] cuda tensor")
    dev = frames[0].device if F else "cuda"
    if out is None:
        out = torch.empty((max(V, 1), 3, out_h, out_w), dtype=torch.float32, device=dev)
    L = lib()
    oh = (C.c_int * max(F, 1))(*[int(f.shape[0]) for f in frames])
    ow = (C.c_int * max(F, 1))(*[int(f.shape[1]) for f in frames])
    ptrs = (C.c_void_p * max(F, 1))(*[f.data_ptr() for f in frames])
    va = view_array(views)
    wb = L.mscnn_preprocess_views_workspace_bytes(va, V, out_h, out_w)
    if ws is None:
        ws = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
    m = (C.c_float * 3)(*mean_bgr)
    _check(L.mscnn_preprocess_views_u8_f32(ptrs, oh, ow, F, va, V, _dev(out), out_h, out_w, m, _dev(ws), C.c_size_t(ws.numel()), _stream()))
    torch.cuda.current_stream().synchronize()     # ws dies with this batch
    return out


def nms_greedy(boxes_xywh, thr, mode="IOU"):
    n = boxes_xywh.shape[0]
    keep = torch.zeros(max(n, 1), dtype=torch.uint8, device=boxes_xywh.device)
    wb = lib().mscnn_nms_workspace_bytes(n)
    ws = torch.empty(wb, dtype=torch.uint8, device=boxes_xywh.device)
    _check(lib().mscnn_nms_greedy_f32(_dev(boxes_xywh), n, thr, NMS_MODES[mode], _dev(keep), _dev(ws), wb, _stream()))
    return keep[:n].bool()


def decode_bbox(bbox, prior, mean=(0, 0, 0, 0), std=(1, 1, 1, 1)):
    R = bbox.shape[0]
    out = torch.empty((R, 5), dtype=torch.float32, device=bbox.device)
    m = (C.c_float * 4)(*mean); s = (C.c_float * 4)(*std)
    _check(lib().mscnn_decodebbox_fwd_f32(_dev(bbox), _dev(prior), _dev(out), R, bbox.shape[1], m, s, _stream()))
    return out


def detections(bbox_pred, cls_pred, props, cls_id, bbox_mean=(0, 0, 0, 0), bbox_std=(0.1, 0.1, 0.2, 0.2),
               proposal_thr=-10.0, ratios=(1.0, 1.0), org_hw=(375, 1242), nms_overlap=0.5, nms=None):
    """nms: None (the existing entry point), an NmsParams or a dict of nms_params() arguments (mscnn_detections_nms_fwd)."""
    R = props.shape[0]
    d = DetectionsDesc()
    _fill_desc(d, cls_pred.shape[1], dict(cls_id=cls_id, bbox_mean=bbox_mean, bbox_std=bbox_std, proposal_thr=proposal_thr, ratios=ratios,
                                          org_hw=org_hw, nms_overlap=nms_overlap))
    dev = props.device
    dets = torch.zeros((max(R, 1), 5), dtype=torch.float64, device=dev)
    ids = torch.zeros(max(R, 1), dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    wb = lib().mscnn_detections_workspace_bytes(R)
    ws = torch.empty(wb, dtype=torch.uint8, device=dev)
    if nms is None:
        _check(lib().mscnn_detections_fwd(C.byref(d), _dev(bbox_pred), _dev(cls_pred), _dev(props), R, _dev(dets), _dev(ids),
                                          _dev(count), _dev(ws), wb, _stream()))
    else:
        _check(lib().mscnn_detections_nms_fwd(C.byref(d), _nms_ref(nms), _dev(bbox_pred), _dev(cls_pred), _dev(props), R, _dev(dets),
                                              _dev(ids), _dev(count), _dev(ws), wb, _stream()))
    D = int(count.item())
    return dets[:D], ids[:D]


def _read_multi_pack(pack, S, K, R, cap, name):
    """The multi pack (mscnn_hip.h) read back: [(dets[D,5], ids relative to row0, row0, rows)] per segment, (None, None, row0, rows)
    for a segment whose image has more rows than max_rows_per_image.  K: slots per image."""
    h = pack.cpu().numpy()
    table = 16 * (S + 1)
    hdr = h[:table].view(np.int32).reshape(S + 1, 4)
    if list(hdr[0]) != [S, R, cap, 0]:
        raise MscnnError(f"{name}: pack header {hdr[0].tolist()}")
    dets = h[table:table + 40 * max(cap, 1)].view(np.float64).reshape(-1, 5)
    ids = h[table + 40 * max(cap, 1):table + 44 * max(cap, 1)].view(np.int32)
    out = []
    for s in range(S):
        cnt, rows, row0, _ = (int(v) for v in hdr[1 + s])
        slot = K * row0 + (s % K) * rows
        out.append((dets[slot:slot + cnt].copy(), ids[slot:slot + cnt].copy(), row0, rows) if cnt >= 0 else (None, None, row0, rows))
    return out


def detections_multi(bbox_pred, cls_pred, props, num_images, segments, max_rows_per_image=None, nms=None, raw_pack=False):
    """Every (image, class) segment in one pass (mscnn_detections_multi_fwd).  props: ROI rows grouped by image, image index in
    column 0; segments: num_images * C dicts of detections() keyword arguments (cls_id, ratios, org_hw, ...), image-major.
    nms: None (mscnn_detections_multi_fwd), an NmsParams or a dict of nms_params() arguments (mscnn_detections_multi_nms_fwd), one
    setting for all segments.  Returns [(dets[D,5], ids relative to row0, row0, rows)] per segment; raw_pack: (that, the pack's
    bytes as a numpy array -- it was zero-filled before the call)."""
    R = props.shape[0]
    S = len(segments)
    Cn = S // num_images
    if Cn * num_images != S:
        raise MscnnError(f"detections_multi: {S} segments for {num_images} images")
    descs = (DetectionsDesc * S)()
    for s, kw in enumerate(segments):
        _fill_desc(descs[s], cls_pred.shape[1], kw)
    M = R if max_rows_per_image is None else max_rows_per_image
    cap = Cn * R
    dev = props.device
    pack = torch.zeros(lib().mscnn_detections_multi_pack_bytes(S, cap), dtype=torch.uint8, device=dev)
    wb = lib().mscnn_detections_multi_workspace_bytes(S, M)
    ws = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
    if nms is None:
        _check(lib().mscnn_detections_multi_fwd(descs, num_images, Cn, _dev(bbox_pred), _dev(cls_pred), _dev(props), R, M, _dev(pack), cap,
                                                _dev(ws), C.c_size_t(wb), _stream()))
    else:
        _check(lib().mscnn_detections_multi_nms_fwd(descs, _nms_ref(nms), num_images, Cn, _dev(bbox_pred), _dev(cls_pred), _dev(props), R, M,
                                                    _dev(pack), cap, _dev(ws), C.c_size_t(wb), _stream()))
    out = _read_multi_pack(pack, S, Cn, R, cap, "detections_multi")
    return (out, pack.cpu().numpy()) if raw_pack else out


def proposals_multi(props, images, raw_pack=False, pack=None):
    """The proposal half of the scripts' result for every image in one pass (mscnn_proposals_multi_fwd).  props: [R, 6] cuda tensor,
    BoxOutput's proposals_score layout, rows grouped by image; images: one dict per image, ratios=(ratio_h, ratio_w) and optionally
    proposal_thr (-10).  Returns [(props[n,5] float64 x y w h score, rows relative to row0, row0, rows)] per image; raw_pack: (that,
    the pack's bytes as a numpy array).  pack: a uint8 cuda tensor to write into (at least the pack's bytes; default: a zero-filled
    one of exactly that size) -- what lies behind the pack's bytes is the caller's."""
    R = props.shape[0]
    B = len(images)
    descs = (ProposalsDesc * max(B, 1))()
    for i, kw in enumerate(images):
        descs[i].proposal_thr = kw.get("proposal_thr", -10.0)
        descs[i].ratio_h, descs[i].ratio_w = kw.get("ratios", (1.0, 1.0))
    cap = R
    nbytes = lib().mscnn_proposals_multi_pack_bytes(B, cap)
    if pack is None:
        pack = torch.zeros(nbytes, dtype=torch.uint8, device=props.device)
    elif pack.numel() < nbytes or pack.dtype != torch.uint8:
        raise MscnnError(f"proposals_multi: the pack needs {nbytes} uint8, got {pack.numel()} {pack.dtype}")
    _check(lib().mscnn_proposals_multi_fwd(descs, B, _dev(props), R, _dev(pack), cap, _stream()))
    out = _read_multi_pack(pack[:nbytes], B, 1, R, cap, "proposals_multi")
    return (out, pack.cpu().numpy()) if raw_pack else out


ROIS_NET, ROIS_IMAGE = 0, 1                                       # mscnn_rois_ingest_f32's coords
ROIS_BAD_NONFINITE, ROIS_BAD_IMAGE, ROIS_BAD_ORDER = 1, 2, 3      # ... and the reasons of its status word
ROIS_MAX_RATIO_IMAGES = 128


def rois_ingest(rows, coords, num_images, ratios=None, with_props=True):
    """Caller-supplied ROIs as BoxOutput's two blobs (mscnn_rois_ingest_f32).  rows: [R, 6] cuda tensor -- float32
    [image x1 y1 x2 y2 score] for ROIS_NET, float64 [image x y w h score] for ROIS_IMAGE with ratios = [(ratio_h, ratio_w)] per image.
    Returns (rois [R, 5], props [R, 6] or None, image_rows [N], status [4]) as numpy arrays after one synchronisation; rois and props
    start as NaN and image_rows as -1, so what a refused list left unwritten shows."""
    R = int(rows.shape[0])
    want = torch.float64 if coords == ROIS_IMAGE else torch.float32
    if rows.dtype != want or rows.dim() != 2 or rows.shape[1] != 6:
        raise MscnnError(f"rois_ingest: rows must be [R, 6] {want}, got {tuple(rows.shape)} {rows.dtype}")
    rois = torch.full((max(R, 1), 5), float("nan"), dtype=torch.float32, device=rows.device)
    props = torch.full((max(R, 1), 6), float("nan"), dtype=torch.float32, device=rows.device) if with_props else None
    image_rows = torch.full((max(num_images, 1),), -1, dtype=torch.int32, device=rows.device)
    status = torch.full((4,), -1, dtype=torch.int32, device=rows.device)
    rh = rw = None
    if ratios is not None:
        rh = (C.c_double * max(len(ratios), 1))(*[float(r[0]) for r in ratios])
        rw = (C.c_double * max(len(ratios), 1))(*[float(r[1]) for r in ratios])
    _check(lib().mscnn_rois_ingest_f32(_dev(rows), coords, R, num_images, rh, rw, _dev(rois), _dev(props), _dev(image_rows), _dev(status),
                                       _stream()))
    torch.cuda.synchronize()
    return (rois.cpu().numpy(), None if props is None else props.cpu().numpy(), image_rows.cpu().numpy(), status.cpu().numpy())


class CascadeOutput(C.Structure):
    """mscnn_cascade_output: the blob triple of one cascade output + its probability columns."""
    _fields_ = [("boxes", C.c_void_p), ("cls_prob", C.c_void_p), ("props", C.c_void_p), ("ncls", C.c_int)]


def detections_cascade_multi(outputs, num_images, segments, det_thr=0.0, max_rows_per_image=None, nms=None, raw_pack=False):
    """Every (image, cascade output, class) segment in one pass (mscnn_detections_cascade_multi_fwd).  outputs: [(boxes [R, 5],
    cls_prob [R, ncls], props [R, 5])] per cascade output, rows grouped by image (image index in column 0 of props); segments:
    num_images * O * C dicts of detections_cascade() keyword arguments (cls_id, ratios, org_hw, nms_overlap), image-major, then
    output, then class.  Returns [(dets[D,5], ids relative to row0, row0, rows)] per segment ((None, None, row0, rows): the image
    has more rows than max_rows_per_image).  nms, raw_pack: as detections_multi (mscnn_detections_cascade_multi_nms_fwd)."""
    O = len(outputs)
    S = len(segments)
    K = S // num_images
    Cn = K // max(O, 1)
    if O < 1 or Cn * O * num_images != S:
        raise MscnnError(f"detections_cascade_multi: {S} segments for {num_images} images x {O} outputs")
    R = outputs[0][2].shape[0]
    outs = (CascadeOutput * O)()
    for o, (boxes, cls_prob, props) in enumerate(outputs):
        if boxes.shape != (R, 5) or props.shape != (R, 5) or cls_prob.shape[0] != R:
            raise MscnnError(f"detections_cascade_multi: output {o}: shapes {tuple(boxes.shape)} {tuple(cls_prob.shape)} {tuple(props.shape)}")
        outs[o].boxes, outs[o].cls_prob, outs[o].props, outs[o].ncls = _dev(boxes).value, _dev(cls_prob).value, _dev(props).value, cls_prob.shape[1]
    descs = (DetectionsDesc * S)()
    for s, kw in enumerate(segments):      # (of the desc, the cascade stage reads ncls, cls_id, ratio_*, org_* and nms_overlap)
        _fill_desc(descs[s], outs[(s % K) // Cn].ncls, kw)
    M = R if max_rows_per_image is None else max_rows_per_image
    cap = K * R
    dev = outputs[0][2].device
    pack = torch.zeros(lib().mscnn_detections_multi_pack_bytes(S, cap), dtype=torch.uint8, device=dev)
    wb = lib().mscnn_detections_cascade_multi_workspace_bytes(S, M)
    ws = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
    if nms is None:
        _check(lib().mscnn_detections_cascade_multi_fwd(descs, C.c_float(det_thr), num_images, O, Cn, outs, R, M, _dev(pack), cap, _dev(ws),
                                                        C.c_size_t(wb), _stream()))
    else:
        _check(lib().mscnn_detections_cascade_multi_nms_fwd(descs, C.c_float(det_thr), _nms_ref(nms), num_images, O, Cn, outs, R, M, _dev(pack),
                                                            cap, _dev(ws), C.c_size_t(wb), _stream()))
    out = _read_multi_pack(pack, S, K, R, cap, "detections_cascade_multi")
    return (out, pack.cpu().numpy()) if raw_pack else out


# ---- several forwards of an image, one NMS (mscnn_detections_candidates_*, mscnn_detections_merge_fwd) ----
class DetectionsView(C.Structure):
    """mscnn_detections_view: where a forward's view of an image lies in the original image."""
    _fields_ = [("off_x", C.c_double), ("off_y", C.c_double), ("flip_x", C.c_int)]


class VoteParams(C.Structure):
    """mscnn_vote_params: the overlap threshold of the box vote, 0 < thr < 1."""
    _fields_ = [("thr", C.c_double)]


SOFT_NMS_METHODS = {"linear": 1, "gaussian": 2}      # MSCNN_SOFT_NMS_LINEAR / _GAUSSIAN


class SoftNmsParams(C.Structure):
    """mscnn_soft_nms_params: method 1 = linear, 2 = gaussian; sigma (gaussian only) > 0; score_thr >= 0; max_out 0 = no bound."""
    _fields_ = [("method", C.c_int), ("sigma", C.c_double), ("score_thr", C.c_double), ("max_out", C.c_int)]


def soft_nms_method(method):
    """A method's number from its name ("linear", "gaussian"); a number passes through for the library to judge."""
    if isinstance(method, str):
        if method not in SOFT_NMS_METHODS:
            raise MscnnError(f"soft nms: method {method!r} is none of {sorted(SOFT_NMS_METHODS)}")
        return SOFT_NMS_METHODS[method]
    return int(method)


MATRIX_NMS_METHODS = {"linear": 1, "gaussian": 2}      # MSCNN_MATRIX_NMS_LINEAR / _GAUSSIAN


class MatrixNmsParams(C.Structure):
    """mscnn_matrix_nms_params: method 1 = linear, 2 = gaussian; sigma (gaussian only) > 0; score_thr >= 0; max_out 0 = no bound."""
    _fields_ = [("method", C.c_int), ("sigma", C.c_double), ("score_thr", C.c_double), ("max_out", C.c_int)]


def matrix_nms_method(method):
    """A method's number from its name ("linear", "gaussian"); a number passes through for the library to judge."""
    if isinstance(method, str):
        if method not in MATRIX_NMS_METHODS:
            raise MscnnError(f"matrix nms: method {method!r} is none of {sorted(MATRIX_NMS_METHODS)}")
        return MATRIX_NMS_METHODS[method]
    return int(method)


WBF_CONF_TYPES = {"avg": 1, "max": 2}      # MSCNN_WBF_CONF_AVG / _MAX


class WbfParams(C.Structure):
    """mscnn_wbf_params: thr inside (0, 1); skip_thr >= 0; conf_type 1 = avg, 2 = max; max_out 0 = no bound."""
    _fields_ = [("thr", C.c_double), ("skip_thr", C.c_double), ("conf_type", C.c_int), ("max_out", C.c_int)]


def wbf_conf_type(conf):
    """A confidence type's number from its name ("avg", "max"); a number passes through for the library to judge."""
    if isinstance(conf, str):
        if conf not in WBF_CONF_TYPES:
            raise MscnnError(f"wbf: conf {conf!r} is none of {sorted(WBF_CONF_TYPES)}")
        return WBF_CONF_TYPES[conf]
    return int(conf)


SEQ_NMS_RESCORES = {"avg": 1, "max": 2}      # MSCNN_SEQ_NMS_AVG / _MAX


class SeqNmsParams(C.Structure):
    """mscnn_seq_nms_params: link_thr inside (0, 1); score_thr >= 0; top_k in [1, 1024]; rescore 1 = avg, 2 = max; max_out 0 = no bound."""
    _fields_ = [("link_thr", C.c_double), ("score_thr", C.c_double), ("top_k", C.c_int), ("rescore", C.c_int), ("max_out", C.c_int)]


def seq_nms_rescore(rescore):
    """A rescoring's number from its name ("avg", "max"); a number passes through for the library to judge."""
    if isinstance(rescore, str):
        if rescore not in SEQ_NMS_RESCORES:
            raise MscnnError(f"seq nms: rescore {rescore!r} is none of {sorted(SEQ_NMS_RESCORES)}")
        return SEQ_NMS_RESCORES[rescore]
    return int(rescore)


def _view_array(views, num_images):
    """views: None (NULL, the identity) or one (off_x, off_y, flip_x) per image."""
    if views is None:
        return None
    if len(views) != num_images:
        raise MscnnError(f"candidates: {len(views)} views for {num_images} images")
    arr = (DetectionsView * max(num_images, 1))()
    for i, (ox, oy, fl) in enumerate(views):
        arr[i].off_x, arr[i].off_y, arr[i].flip_x = float(ox), float(oy), int(fl)
    return arr


class Candidates:
    """The candidate lists of S segments with cand_cap slots each: reset on creation; add() / cascade_add() after each forward (the
    pass index counts them), merge() runs the NMS over each list.  Every buffer comes from `torch` of this module."""

    def __init__(self, num_segments, cand_cap, device="cuda"):
        self.S, self.cap, self.passes = num_segments, cand_cap, 0
        nbytes = lib().mscnn_detections_candidates_bytes(num_segments, cand_cap)
        if nbytes == 0:
            raise MscnnError(f"candidates: {num_segments} segments x {cand_cap} slots")
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _check(lib().mscnn_detections_candidates_reset(_dev(self.buf), num_segments, cand_cap, _stream()))
        self.overlap = None

    def _descs(self, segments, ncls_of):
        if len(segments) != self.S:
            raise MscnnError(f"candidates: {len(segments)} segments, the lists were made for {self.S}")
        descs = (DetectionsDesc * self.S)()
        for s, kw in enumerate(segments):
            _fill_desc(descs[s], ncls_of(s), kw)
        if self.overlap is None:
            self.overlap = [d.nms_overlap for d in descs]
        return descs

    def add(self, bbox_pred, cls_pred, props, num_images, segments, views=None, nms=NMS_NULL, pass_index=None):
        """mscnn_detections_candidates_add: segments as in detections_multi; views: None or [(off_x, off_y, flip_x)] per image."""
        descs = self._descs(segments, lambda s: cls_pred.shape[1])
        k = self.passes if pass_index is None else pass_index
        _check(lib().mscnn_detections_candidates_add(descs, _view_array(views, num_images), _nms_ref(nms), k, num_images, self.S // num_images,
                                                     _dev(bbox_pred), _dev(cls_pred), _dev(props), props.shape[0], _dev(self.buf), self.cap,
                                                     _stream()))
        self.passes += 1

    def cascade_add(self, outputs, num_images, segments, det_thr=0.0, views=None, nms=NMS_NULL, pass_index=None):
        """mscnn_detections_candidates_cascade_add: outputs and segments as in detections_cascade_multi."""
        O = len(outputs)
        K = self.S // num_images
        Cn = K // max(O, 1)
        outs = (CascadeOutput * max(O, 1))()
        for o, (boxes, cls_prob, props) in enumerate(outputs):
            outs[o].boxes, outs[o].cls_prob, outs[o].props, outs[o].ncls = _dev(boxes).value, _dev(cls_prob).value, _dev(props).value, cls_prob.shape[1]
        descs = self._descs(segments, lambda s: outs[(s % K) // Cn].ncls)
        k = self.passes if pass_index is None else pass_index
        _check(lib().mscnn_detections_candidates_cascade_add(descs, _view_array(views, num_images), C.c_float(det_thr), _nms_ref(nms), k,
                                                             num_images, O, Cn, outs, outputs[0][2].shape[0], _dev(self.buf), self.cap, _stream()))
        self.passes += 1

    def _view_descs(self, segments, ncls_of, num_images, list_of):
        """The descs of the views forms: one per (image, slot) of THIS forward, K = slots per image; S = frames x K.  A list's overlap
        for merge() is the one of the first image that reached it (0.5 for a list nothing reached)."""
        K = len(segments) // max(num_images, 1)
        if K < 1 or len(segments) != num_images * K or len(list_of) != num_images or self.S % K:
            raise MscnnError(f"candidates: {len(segments)} segments and {len(list_of)} list_of entries for {num_images} images, {self.S} lists")
        descs = (DetectionsDesc * len(segments))()
        for s, kw in enumerate(segments):
            _fill_desc(descs[s], ncls_of(s % K), kw)
        if self.overlap is None:
            self.overlap, self._overlap_known = [0.5] * self.S, set()
        for s in range(len(segments)):
            l = list_of[s // K] * K + s % K
            if 0 <= l < self.S and l not in self._overlap_known:
                self.overlap[l] = descs[s].nms_overlap
                self._overlap_known.add(l)
        return descs, K

    def add_views(self, bbox_pred, cls_pred, props, num_images, segments, list_of, views=None, nms=NMS_NULL, pass_index=None):
        """mscnn_detections_candidates_add_views: the images of ONE batched forward into the lists of their frames.  segments: one dict
        per (image, class) of this forward; list_of: the frame of each image; the lists were made for frames x classes segments."""
        descs, K = self._view_descs(segments, lambda k: cls_pred.shape[1], num_images, list_of)
        k = self.passes if pass_index is None else pass_index
        lo = (C.c_int * num_images)(*[int(v) for v in list_of])
        _check(lib().mscnn_detections_candidates_add_views(descs, _view_array(views, num_images), lo, _nms_ref(nms), k, num_images,
                                                           self.S // K, K, _dev(bbox_pred), _dev(cls_pred), _dev(props), props.shape[0],
                                                           _dev(self.buf), self.cap, _stream()))
        self.passes += 1

    def cascade_add_views(self, outputs, num_images, segments, list_of, det_thr=0.0, views=None, nms=NMS_NULL, pass_index=None):
        """mscnn_detections_candidates_cascade_add_views: outputs and segments as in cascade_add, for the images of this forward."""
        O = len(outputs)
        outs = (CascadeOutput * max(O, 1))()
        for o, (boxes, cls_prob, props) in enumerate(outputs):
            outs[o].boxes, outs[o].cls_prob, outs[o].props, outs[o].ncls = _dev(boxes).value, _dev(cls_prob).value, _dev(props).value, cls_prob.shape[1]
        Cn = len(segments) // max(num_images * O, 1)
        descs, K = self._view_descs(segments, lambda k: outs[k // max(Cn, 1)].ncls, num_images, list_of)
        k = self.passes if pass_index is None else pass_index
        lo = (C.c_int * num_images)(*[int(v) for v in list_of])
        _check(lib().mscnn_detections_candidates_cascade_add_views(descs, _view_array(views, num_images), lo, C.c_float(det_thr), _nms_ref(nms), k,
                                                                   num_images, self.S // K, O, Cn, outs, outputs[0][2].shape[0], _dev(self.buf),
                                                                   self.cap, _stream()))
        self.passes += 1

    def counts(self):
        """[(rows that wanted in, overflow flag)] per segment, read from the device."""
        return self.buf[:8 * self.S].cpu().numpy().view(np.int32).reshape(self.S, 2).tolist()

    def vote(self, pack, thr):
        """mscnn_detections_merge_vote_fwd on the device pack a merge() of these lists filled: every kept row's box becomes the
        prob-weighted mean of the list's candidates whose union overlap with it is >= thr, in place.  Not idempotent."""
        _check(lib().mscnn_detections_merge_vote_fwd(C.byref(VoteParams(float(thr))), self.S, _dev(self.buf), self.cap, _dev(pack), _stream()))

    def merge(self, nms=NMS_NULL, nms_overlap=None, raw_pack=False, pack=None, ws=None, vote_thr=None):
        """mscnn_detections_merge_fwd.  Returns [(dets[D,5], tags[D], candidates)] per segment ((None, None, candidates): the list
        overflowed); raw_pack: (that, the pack's bytes as a numpy array -- zero-filled before the call unless `pack` is given).
        vote_thr: vote(pack, vote_thr) runs on the pack before it is read."""
        S, cap = self.S, self.cap
        ov = self.overlap if nms_overlap is None else nms_overlap
        ov = (C.c_double * S)(*[float(v) for v in (ov if ov is not None else [0.5] * S)])
        nbytes = lib().mscnn_detections_multi_pack_bytes(S, S * cap)
        if pack is None:
            pack = torch.zeros(nbytes, dtype=torch.uint8, device=self.buf.device)
        wb = lib().mscnn_detections_merge_workspace_bytes(S, cap)
        if ws is None:
            ws = torch.empty(max(wb, 1), dtype=torch.uint8, device=self.buf.device)
        _check(lib().mscnn_detections_merge_fwd(ov, _nms_ref(nms), S, _dev(self.buf), cap, _dev(pack), _dev(ws), C.c_size_t(ws.numel()),
                                                _stream()))
        if vote_thr is not None:
            self.vote(pack, vote_thr)
        return self._read_pack(pack, nbytes, raw_pack, "detections_merge")

    def merge_soft(self, method, sigma=0.5, score_thr=0.001, max_out=0, nms_overlap=None, raw_pack=False, pack=None, ws=None, vote_thr=None):
        """mscnn_detections_merge_soft_fwd: Soft-NMS over each list in place of merge()'s hard NMS -- method "linear" (decay by 1 - IoU
        above the list's nms_overlap) or "gaussian" (by exp(-IoU^2 / sigma)); picks until the best live score is below score_thr or,
        with max_out > 0, max_out are out.  Returns what merge() returns, the rows in pick order with their decayed scores."""
        S, cap = self.S, self.cap
        ov = self.overlap if nms_overlap is None else nms_overlap
        ov = (C.c_double * S)(*[float(v) for v in (ov if ov is not None else [0.5] * S)])
        nbytes = lib().mscnn_detections_multi_pack_bytes(S, S * cap)
        if pack is None:
            pack = torch.zeros(nbytes, dtype=torch.uint8, device=self.buf.device)
        wb = lib().mscnn_detections_merge_soft_workspace_bytes(S, cap)
        if ws is None:
            ws = torch.empty(max(wb, 1), dtype=torch.uint8, device=self.buf.device)
        soft = SoftNmsParams(soft_nms_method(method), float(sigma), float(score_thr), int(max_out))
        _check(lib().mscnn_detections_merge_soft_fwd(ov, C.byref(soft), S, _dev(self.buf), cap, _dev(pack), _dev(ws), C.c_size_t(ws.numel()),
                                                     _stream()))
        if vote_thr is not None:
            self.vote(pack, vote_thr)
        return self._read_pack(pack, nbytes, raw_pack, "detections_merge_soft")

    def merge_matrix(self, method, sigma=0.5, score_thr=0.001, max_out=0, raw_pack=False, pack=None, ws=None, vote_thr=None):
        """mscnn_detections_merge_matrix_fwd: Matrix NMS over each list in place of merge()'s hard NMS -- every score decayed by its
        worst compensated overlap with a higher-ranked candidate, method "linear" (min (1 - IoU) / (1 - comp)) or "gaussian"
        (exp(-max (IoU^2 - comp^2) / sigma)), no pick loop; the candidates with score' >= score_thr, the first max_out of them when
        max_out > 0.  Returns what merge() returns, the rows in descending score' order.  No nms_overlap is read."""
        S, cap = self.S, self.cap
        nbytes = lib().mscnn_detections_multi_pack_bytes(S, S * cap)
        if pack is None:
            pack = torch.zeros(nbytes, dtype=torch.uint8, device=self.buf.device)
        wb = lib().mscnn_detections_merge_matrix_workspace_bytes(S, cap)
        if ws is None:
            ws = torch.empty(max(wb, 1), dtype=torch.uint8, device=self.buf.device)
        mx = MatrixNmsParams(matrix_nms_method(method), float(sigma), float(score_thr), int(max_out))
        _check(lib().mscnn_detections_merge_matrix_fwd(C.byref(mx), S, _dev(self.buf), cap, _dev(pack), _dev(ws), C.c_size_t(ws.numel()),
                                                       _stream()))
        if vote_thr is not None:
            self.vote(pack, vote_thr)
        return self._read_pack(pack, nbytes, raw_pack, "detections_merge_matrix")

    def merge_wbf(self, thr, skip_thr=0.0, conf="avg", expected=1, max_out=0, raw_pack=False, pack=None, ws=None, members=None):
        """mscnn_detections_merge_wbf_fwd: weighted boxes fusion over each list in place of merge()'s hard NMS -- the candidates with a
        score >= skip_thr walked in score order into clusters (union overlap with the cluster's fused box > thr), a cluster's box the
        score-weighted mean of its members, its confidence their mean ("avg") or largest ("max") score times min(members, expected) /
        expected; expected: one int for every list or one per list.  Returns (what merge() returns -- the rows in descending confidence,
        the tag the first member's --, [members[D] int32 per segment, None for an overflowed list]).  members: an int32 device tensor of
        S * cand_cap entries to use (zero-filled otherwise).  No nms_overlap is read."""
        S, cap = self.S, self.cap
        nbytes = lib().mscnn_detections_multi_pack_bytes(S, S * cap)
        if pack is None:
            pack = torch.zeros(nbytes, dtype=torch.uint8, device=self.buf.device)
        wb = lib().mscnn_detections_merge_wbf_workspace_bytes(S, cap)
        if ws is None:
            ws = torch.empty(max(wb, 1), dtype=torch.uint8, device=self.buf.device)
        if members is None:
            members = torch.zeros(S * cap, dtype=torch.int32, device=self.buf.device)
        ex = (C.c_int * S)(*([int(expected)] * S if isinstance(expected, int) else [int(v) for v in expected]))
        wbf = WbfParams(float(thr), float(skip_thr), wbf_conf_type(conf), int(max_out))
        _check(lib().mscnn_detections_merge_wbf_fwd(C.byref(wbf), ex, S, _dev(self.buf), cap, _dev(pack), _dev(members), _dev(ws),
                                                    C.c_size_t(ws.numel()), _stream()))
        out = self._read_pack(pack, nbytes, raw_pack, "detections_merge_wbf")
        mh = members.cpu().numpy().reshape(S, cap)
        segs = out[0] if raw_pack else out
        return out, [None if d is None else mh[s, :len(d)].copy() for s, (d, _, _) in enumerate(segs)]

    def merge_seq(self, link_thr, num_frames, score_thr=0.001, top_k=300, rescore="avg", max_out=0, nms_overlap=None, raw_pack=False,
                  pack=None, ws=None, seq=None, vote_thr=None):
        """mscnn_detections_merge_seq_fwd: Seq-NMS in place of merge()'s hard NMS -- the lists are the num_frames consecutive frames of
        one clip (list = frame x K + slot): per slot, the boxes of neighbouring frames with a union overlap > link_thr are linked, the
        chain with the largest score sum comes out with its mean ("avg") or largest ("max") score on every box and suppresses what its
        boxes overlap (the list's nms_overlap) in their own frames, until no box is left.  Of each list the leading candidates with a
        score >= score_thr take part, at most top_k.  Returns (what merge() returns -- the rows in descending score' --, [seq[D] int32
        per segment, None for an overflowed list]): seq is the sequence (tubelet) id, unique within a slot.  seq: an int32 device
        tensor of S * cand_cap entries to use (zero-filled otherwise), or False for the op's NULL (then the second result is None).
        vote_thr: vote(pack, vote_thr) runs on the pack before it is read."""
        S, cap = self.S, self.cap
        if num_frames < 1 or S % num_frames:
            raise MscnnError(f"candidates: {S} lists are not {num_frames} frames of equally many slots")
        ov = self.overlap if nms_overlap is None else nms_overlap
        ov = (C.c_double * S)(*[float(v) for v in (ov if ov is not None else [0.5] * S)])
        nbytes = lib().mscnn_detections_multi_pack_bytes(S, S * cap)
        if pack is None:
            pack = torch.zeros(nbytes, dtype=torch.uint8, device=self.buf.device)
        sq = SeqNmsParams(float(link_thr), float(score_thr), int(top_k), seq_nms_rescore(rescore), int(max_out))
        wb = lib().mscnn_detections_merge_seq_workspace_bytes(num_frames, S // num_frames, cap, sq.top_k)
        if ws is None:
            ws = torch.empty(max(wb, 1), dtype=torch.uint8, device=self.buf.device)
        if seq is None:
            seq = torch.zeros(S * cap, dtype=torch.int32, device=self.buf.device)
        _check(lib().mscnn_detections_merge_seq_fwd(ov, C.byref(sq), num_frames, S // num_frames, _dev(self.buf), cap, _dev(pack),
                                                    None if seq is False else _dev(seq), _dev(ws), C.c_size_t(ws.numel()), _stream()))
        if vote_thr is not None:
            self.vote(pack, vote_thr)
        out = self._read_pack(pack, nbytes, raw_pack, "detections_merge_seq")
        if seq is False:
            return out, None
        sh = seq.cpu().numpy().reshape(S, cap)
        segs = out[0] if raw_pack else out
        return out, [None if d is None else sh[s, :len(d)].copy() for s, (d, _, _) in enumerate(segs)]

    def _read_pack(self, pack, nbytes, raw_pack, what):
        """The merge's multi pack on the host: [(dets, tags, candidates)] per segment, with raw_pack also its bytes."""
        S, cap = self.S, self.cap
        h = pack[:nbytes].cpu().numpy()
        table = 16 * (S + 1)
        hdr = h[:table].view(np.int32).reshape(S + 1, 4)
        if list(hdr[0]) != [S, cap, S * cap, 0]:
            raise MscnnError(f"{what}: pack header {hdr[0].tolist()}")
        dets = h[table:table + 40 * S * cap].view(np.float64).reshape(-1, 5)
        tags = h[table + 40 * S * cap:table + 44 * S * cap].view(np.int32)
        out = []
        for s in range(S):
            cnt, cands, row0, zero = (int(v) for v in hdr[1 + s])
            if row0 != s * cap or zero != 0:
                raise MscnnError(f"{what}: table entry {s}: {hdr[1 + s].tolist()}")
            out.append((dets[row0:row0 + cnt].copy(), tags[row0:row0 + cnt].copy(), cands) if cnt >= 0 else (None, None, cands))
        return (out, h) if raw_pack else out


# ---- the tracker behind the final stage (mscnn_hip.h: mscnn_tracks_update_fwd) ----
TRACK_MOTIONS = {"none": 1, "linear": 2}      # MSCNN_TRACK_MOTION_NONE / _LINEAR
TRACKS_HEADER_WORDS = 8                       # MSCNN_TRACKS_HEADER_WORDS: {n, next_id, frame, dropped, skipped, 0, 0, 0}
TRACKS_MAX = 1024                             # max_tracks' bound, and the detections of a frame that enter


class TrackParams(C.Structure):
    """mscnn_track_params: low_thr <= high_thr <= new_thr; match_thr, match_thr_low inside [0, 1); vel_gain inside (0, 1]; motion 1 =
    none, 2 = linear; max_age >= 0; min_hits >= 1."""
    _fields_ = [("high_thr", C.c_double), ("low_thr", C.c_double), ("new_thr", C.c_double), ("match_thr", C.c_double),
                ("match_thr_low", C.c_double), ("vel_gain", C.c_double), ("motion", C.c_int), ("max_age", C.c_int), ("min_hits", C.c_int)]


class TrackRecord(C.Structure):
    """mscnn_track_record (104 bytes)."""
    _fields_ = [("box", C.c_double * 4), ("obs", C.c_double * 4), ("vel", C.c_double * 2), ("score", C.c_double), ("id", C.c_int32),
                ("hits", C.c_int32), ("misses", C.c_int32), ("confirmed", C.c_int32)]


TRACK_RECORD = np.dtype([("box", "<f8", 4), ("obs", "<f8", 4), ("vel", "<f8", 2), ("score", "<f8"), ("id", "<i4"), ("hits", "<i4"),
                         ("misses", "<i4"), ("confirmed", "<i4")])
assert TRACK_RECORD.itemsize == C.sizeof(TrackRecord) == 104


def track_motion(motion):
    """A motion's number from its name ("none", "linear"); a number passes through for the library to judge."""
    if isinstance(motion, str):
        if motion not in TRACK_MOTIONS:
            raise MscnnError(f"tracker: motion {motion!r} is none of {sorted(TRACK_MOTIONS)}")
        return TRACK_MOTIONS[motion]
    return int(motion)


def track_params(high_thr=0.5, low_thr=0.1, new_thr=None, match_thr=0.3, match_thr_low=0.5, motion="linear", vel_gain=0.5, max_age=30,
                 min_hits=1):
    """A TrackParams; new_thr None: high_thr."""
    return TrackParams(float(high_thr), float(low_thr), float(high_thr if new_thr is None else new_thr), float(match_thr),
                       float(match_thr_low), float(vel_gain), track_motion(motion), int(max_age), int(min_hits))


def tracks_state_layout(num_slots, max_tracks):
    """mscnn_tracks_state_layout_of: (byte offset of a slot's records, bytes of a record, of a slot, of the state)."""
    slot = 4 * TRACKS_HEADER_WORDS + max(max_tracks, 0) * TRACK_RECORD.itemsize
    return 4 * TRACKS_HEADER_WORDS, TRACK_RECORD.itemsize, slot, (max(num_slots, 0) * slot + 15) // 16 * 16


def tracks_state_parse(state, num_slots, max_tracks):
    """A state buffer (uint8, host) as one dict per slot: n, next_id, frame, dropped, skipped and tracks = the first n records as a
    numpy record array (box, obs, vel, score, id, hits, misses, confirmed)."""
    rec_at, rec, slot, total = tracks_state_layout(num_slots, max_tracks)
    b = np.ascontiguousarray(state, dtype=np.uint8).reshape(-1)
    if b.size < total:
        raise MscnnError(f"tracker: a state of {b.size} bytes, {num_slots} slots x {max_tracks} tracks need {total}")
    out = []
    for k in range(num_slots):
        h = b[k * slot:k * slot + rec_at].view(np.int32)
        n = int(h[0])
        if not 0 <= n <= max_tracks:
            raise MscnnError(f"tracker: slot {k} holds {n} tracks of {max_tracks} (a state that was never reset?)")
        recs = b[k * slot + rec_at:k * slot + rec_at + n * rec].view(TRACK_RECORD).copy()
        out.append(dict(n=n, next_id=int(h[1]), frame=int(h[2]), dropped=int(h[3]), skipped=int(h[4]), tracks=recs))
    return out


def tracks_state_new(num_slots, max_tracks, device="cuda"):
    """A reset state buffer (uint8 device tensor of mscnn_tracks_state_bytes)."""
    nbytes = lib().mscnn_tracks_state_bytes(num_slots, max_tracks)
    if nbytes == 0:
        raise MscnnError(f"tracker: {num_slots} slots x {max_tracks} tracks (max_tracks inside [1, {TRACKS_MAX}])")
    state = torch.empty(nbytes, dtype=torch.uint8, device=device)
    _check(lib().mscnn_tracks_state_reset(_dev(state), num_slots, max_tracks, _stream()))
    return state


def tracks_update(params, num_frames, num_slots, pack, cap, state_in, max_tracks, state_out=None, ids=None):
    """mscnn_tracks_update_fwd on a multi pack of num_frames x num_slots segments with cap rows (a uint8 device tensor, only read):
    steps the tracks of state_in through the frames into state_out (None: in place) and writes one track id per detection row into
    ids (int32 [cap]; zero-filled when None).  Returns (state_out, ids); a segment's ids start at its row offset."""
    if state_out is None:
        state_out = state_in
    if ids is None:
        ids = torch.zeros(max(cap, 1), dtype=torch.int32, device=pack.device)
    _check(lib().mscnn_tracks_update_fwd(C.byref(params), num_frames, num_slots, _dev(pack), cap, _dev(state_in), _dev(state_out),
                                         max_tracks, _dev(ids), _stream()))
    return state_out, ids


TRACKS_STREAMS_MAX = 256                      # streams of a call, and frames of a call with more than one stream


def tracks_update_streams(params, num_frames, num_slots, num_streams, stream_of, pack, cap, state_in, max_tracks, state_out=None, ids=None):
    """mscnn_tracks_update_streams_fwd: as tracks_update, frame t belonging to stream stream_of[t] (a host sequence of num_frames ints
    inside [0, num_streams)); the state holds num_streams * num_slots tables, (stream s, slot k) at s * num_slots + k.  Every (stream,
    slot) is stepped through its own frames only, all in one launch.  Returns (state_out, ids)."""
    if state_out is None:
        state_out = state_in
    if ids is None:
        ids = torch.zeros(max(cap, 1), dtype=torch.int32, device=pack.device)
    so = np.ascontiguousarray(stream_of, dtype=np.int32).reshape(-1)
    if so.size != num_frames:
        raise MscnnError(f"tracker: stream_of names {so.size} frames, the call has {num_frames}")
    _check(lib().mscnn_tracks_update_streams_fwd(C.byref(params), num_frames, num_slots, num_streams, so.ctypes.data_as(C.c_void_p), _dev(pack),
                                                 cap, _dev(state_in), _dev(state_out), max_tracks, _dev(ids), _stream()))
    return state_out, ids


def tracks_state_reset_slots(state, num_slots_total, max_tracks, first_slot, count):
    """mscnn_tracks_state_reset_slots: resets the tables [first_slot, first_slot + count) of a state of num_slots_total tables (one
    stream of several starts again, the others keep their tracks).  Returns state."""
    _check(lib().mscnn_tracks_state_reset_slots(_dev(state), num_slots_total, max_tracks, first_slot, count, _stream()))
    return state


# ---- the tracker with a Kalman filter per track (mscnn_hip.h: mscnn_tracks_update_kalman_fwd) ----
class TrackKalmanParams(C.Structure):
    """mscnn_track_kalman_params: every std finite and > 0; std_position / std_velocity are times the track's height."""
    _fields_ = [("std_position", C.c_double), ("std_velocity", C.c_double), ("std_aspect", C.c_double), ("std_aspect_velocity", C.c_double),
                ("std_aspect_measure", C.c_double), ("freeze_lost_height", C.c_int)]


class TracksKalmanCall(C.Structure):
    """mscnn_tracks_kalman_call: the one argument of mscnn_tracks_update_kalman_fwd."""
    _fields_ = [("size", C.c_size_t), ("track", C.c_void_p), ("filter", C.c_void_p), ("num_frames", C.c_int), ("num_slots", C.c_int),
                ("num_streams", C.c_int), ("stream_of", C.c_void_p), ("pack_dev", C.c_void_p), ("cap", C.c_int), ("state_in", C.c_void_p),
                ("state_out", C.c_void_p), ("filter_in", C.c_void_p), ("filter_out", C.c_void_p), ("max_tracks", C.c_int),
                ("track_ids_dev", C.c_void_p), ("stream", C.c_void_p)]


TRACK_KALMAN_RECORD = np.dtype([("x", "<f8", 4), ("v", "<f8", 4), ("p", "<f8", 4), ("q", "<f8", 4), ("r", "<f8", 4)])
assert TRACK_KALMAN_RECORD.itemsize == 160      # mscnn_track_kalman_record


def track_kalman_params(std_position=1 / 20, std_velocity=1 / 160, std_aspect=1e-2, std_aspect_velocity=1e-5, std_aspect_measure=1e-1,
                        freeze_lost_height=True):
    """A TrackKalmanParams with the defaults of SORT / DeepSORT / ByteTrack."""
    return TrackKalmanParams(float(std_position), float(std_velocity), float(std_aspect), float(std_aspect_velocity),
                             float(std_aspect_measure), int(bool(freeze_lost_height)))


def tracks_kalman_state_bytes(num_slots, max_tracks):
    """mscnn_tracks_kalman_state_bytes: the bytes of a filter table beside a state of num_slots tables (0: refused)."""
    return int(lib().mscnn_tracks_kalman_state_bytes(num_slots, max_tracks))


def tracks_update_kalman(params, kparams, num_frames, num_slots, num_streams, stream_of, pack, cap, state_in, filter_in, max_tracks,
                         state_out=None, filter_out=None, ids=None):
    """mscnn_tracks_update_kalman_fwd: as tracks_update_streams with params.motion none and a Kalman filter per track (kparams), its
    records in filter_in / filter_out (uint8 device tensors of tracks_kalman_state_bytes(num_streams * num_slots, max_tracks); None:
    in place) beside the state's.  stream_of may be None with one stream.  Returns (state_out, filter_out, ids)."""
    if state_out is None:
        state_out = state_in
    if filter_out is None:
        filter_out = filter_in
    if ids is None:
        ids = torch.zeros(max(cap, 1), dtype=torch.int32, device=pack.device)
    so = None
    if stream_of is not None:
        so = np.ascontiguousarray(stream_of, dtype=np.int32).reshape(-1)
        if so.size != num_frames:
            raise MscnnError(f"tracker: stream_of names {so.size} frames, the call has {num_frames}")
    def at(t):
        p = _dev(t)
        return None if p is None else p.value
    call = TracksKalmanCall(C.sizeof(TracksKalmanCall), C.addressof(params), C.addressof(kparams), num_frames, num_slots, num_streams,
                            None if so is None else so.ctypes.data, at(pack), cap, at(state_in), at(state_out), at(filter_in),
                            at(filter_out), max_tracks, at(ids), _stream().value)
    _check(lib().mscnn_tracks_update_kalman_fwd(C.byref(call)))
    return state_out, filter_out, ids


# ---- the tracker's matching as a choice (mscnn_hip.h: mscnn_tracks_update_assign_fwd) ----
TRACK_ASSIGNS = {"greedy": 1, "optimal": 2}      # MSCNN_TRACK_ASSIGN_*
TRACKS_STEPS = 5                                 # MSCNN_TRACKS_STEPS: the header word of the optimal form's search steps


class TracksAssignCall(C.Structure):
    """mscnn_tracks_assign_call: the one argument of mscnn_tracks_update_assign_fwd."""
    _fields_ = [("size", C.c_size_t), ("track", C.c_void_p), ("filter", C.c_void_p), ("assign", C.c_int), ("num_frames", C.c_int),
                ("num_slots", C.c_int), ("num_streams", C.c_int), ("stream_of", C.c_void_p), ("pack_dev", C.c_void_p), ("cap", C.c_int),
                ("state_in", C.c_void_p), ("state_out", C.c_void_p), ("filter_in", C.c_void_p), ("filter_out", C.c_void_p),
                ("max_tracks", C.c_int), ("track_ids_dev", C.c_void_p), ("stream", C.c_void_p)]


def track_assign(assign):
    """An assignment's number from its name ("greedy", "optimal"); a number passes through for the library to judge."""
    if isinstance(assign, str):
        if assign not in TRACK_ASSIGNS:
            raise MscnnError(f"tracker: assign {assign!r} is none of {sorted(TRACK_ASSIGNS)}")
        return TRACK_ASSIGNS[assign]
    return int(assign)


def tracks_state_steps(state, num_slots, max_tracks):
    """Header word 5 of every table of a state buffer (uint8, host): the optimal form's running total of search steps."""
    rec_at, _, slot, total = tracks_state_layout(num_slots, max_tracks)
    b = np.ascontiguousarray(state, dtype=np.uint8).reshape(-1)
    if b.size < total:
        raise MscnnError(f"tracker: a state of {b.size} bytes, {num_slots} slots x {max_tracks} tracks need {total}")
    return [int(b[k * slot:k * slot + rec_at].view(np.int32)[TRACKS_STEPS]) for k in range(num_slots)]


def tracks_update_assign(params, kparams, assign, num_frames, num_slots, num_streams, stream_of, pack, cap, state_in, max_tracks,
                         filter_in=None, state_out=None, filter_out=None, ids=None):
    """mscnn_tracks_update_assign_fwd: tracks_update_streams (kparams None) or tracks_update_kalman (kparams and filter tables given)
    with the matching of both passes chosen: "greedy" is the existing op byte for byte, "optimal" the maximum-weight assignment, which
    also counts its search steps into header word 5.  Returns (state_out, filter_out, ids)."""
    if state_out is None:
        state_out = state_in
    if filter_out is None:
        filter_out = filter_in
    if ids is None:
        ids = torch.zeros(max(cap, 1), dtype=torch.int32, device=pack.device)
    so = None
    if stream_of is not None:
        so = np.ascontiguousarray(stream_of, dtype=np.int32).reshape(-1)
        if so.size != num_frames:
            raise MscnnError(f"tracker: stream_of names {so.size} frames, the call has {num_frames}")
    def at(t):
        p = _dev(t)
        return None if p is None else p.value
    call = TracksAssignCall(C.sizeof(TracksAssignCall), C.addressof(params), None if kparams is None else C.addressof(kparams),
                            track_assign(assign), num_frames, num_slots, num_streams, None if so is None else so.ctypes.data, at(pack), cap,
                            at(state_in), at(state_out), at(filter_in), at(filter_out), max_tracks, at(ids), _stream().value)
    _check(lib().mscnn_tracks_update_assign_fwd(C.byref(call)))
    return state_out, filter_out, ids


# ---- the render stage (mscnn_hip.h: mscnn_render_detections_u8) ----
RENDER_LABELS = {"none": 0, "score": 1, "id": 2, "both": 3}
RENDER_COLOR_BY = {"slot": 0, "id": 1}
RENDER_MAX_COLORS = 32


class RenderParams(C.Structure):
    """mscnn_render_params (136 bytes)."""
    _fields_ = [("show_thr", C.c_double), ("thickness", C.c_int), ("outline_alpha", C.c_int), ("fill_alpha", C.c_int), ("label", C.c_int),
                ("label_scale", C.c_int), ("color_by", C.c_int), ("pixelate", C.c_int), ("num_colors", C.c_int),
                ("colors", (C.c_ubyte * 3) * RENDER_MAX_COLORS)]


def render_params(colors, show_thr=0.3, thickness=2, outline_alpha=256, fill_alpha=0, label="score", label_scale=1, color_by="slot", pixelate=0):
    """A RenderParams; label and color_by by name (RENDER_LABELS, RENDER_COLOR_BY) or by number, colors a sequence of 1 .. 32 RGB
    triples.  The values are checked by the op, which names the one it refuses."""
    for name, table, v in (("label", RENDER_LABELS, label), ("color_by", RENDER_COLOR_BY, color_by)):
        if isinstance(v, str) and v not in table:
            raise MscnnError(f"render: {name} {v!r} is none of {sorted(table)}")
    cols = [tuple(int(v) for v in c) for c in colors]
    if len(cols) > RENDER_MAX_COLORS or any(len(c) != 3 or min(c) < 0 or max(c) > 255 for c in cols):
        raise MscnnError(f"render: colors holds {len(cols)} entries (at most {RENDER_MAX_COLORS} RGB triples of 0 .. 255)")
    p = RenderParams(float(show_thr), int(thickness), int(outline_alpha), int(fill_alpha), int(RENDER_LABELS.get(label, label)),
                     int(label_scale), int(RENDER_COLOR_BY.get(color_by, color_by)), int(pixelate), len(cols))
    for i, c in enumerate(cols):
        p.colors[i][:] = c
    return p


def render_glyph_rows(ch):
    """mscnn_render_glyph_rows: the seven rows of the 5 x 7 glyph of ch ('0' .. '9', '.', ' '), bit 4 = the left column.  No device."""
    rows = (C.c_ubyte * 7)()
    _check(lib().mscnn_render_glyph_rows(ord(ch), rows))
    return tuple(rows)


def render_detections(params, frames, num_slots, pack, cap, ids=None, out=None):
    """mscnn_render_detections_u8: the detections of a multi pack of len(frames) x num_slots segments with cap rows (a uint8 device
    tensor) drawn into copies of frames (uint8 [h, w, 3] contiguous cuda tensors, each of its own size); ids: the tracker's int32
    [cap] buffer or None.  out: the tensors to write (None: new ones).  Returns out."""
    B = len(frames)
    if out is None:
        out = [torch.empty_like(f) for f in frames]
    if len(out) != B:
        raise MscnnError(f"render: {len(out)} output frames for {B} frames")
    for b, (f, o) in enumerate(zip(frames, out)):
        for t, what in ((f, "frame"), (o, "output frame")):
            if t.dim() != 3 or t.shape[2] != 3 or t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous():
                raise MscnnError(f"render: {what} {b} is not a contiguous uint8 [H, W, 3] cuda tensor")
        if o.shape != f.shape:
            raise MscnnError(f"render: output frame {b} is {tuple(o.shape)}, the frame {tuple(f.shape)}")
    oh = (C.c_int * max(B, 1))(*[int(f.shape[0]) for f in frames])
    ow = (C.c_int * max(B, 1))(*[int(f.shape[1]) for f in frames])
    src = (C.c_void_p * max(B, 1))(*[f.data_ptr() for f in frames])
    dst = (C.c_void_p * max(B, 1))(*[o.data_ptr() for o in out])
    _check(lib().mscnn_render_detections_u8(C.byref(params), src, dst, oh, ow, B, num_slots, _dev(pack), cap, _dev(ids), _stream()))
    return out


# ---- health of the plane-GEMM kernel's stream-K hand-off (mscnn_hip.h) ----
def wgemm_handoff_event():
    """Tag of the last launch on the current device whose finisher gave up on a contributor (0: none); synchronise first."""
    return int(lib().mscnn_wgemm_handoff_event())


def wgemm_force_whole_tiles(on=True):
    lib().mscnn_wgemm_force_whole_tiles(int(bool(on)))


def wgemm_whole_tiles_forced():
    return bool(lib().mscnn_wgemm_whole_tiles_forced())


def debug_wgemm_handoff_fault(drop_publish=False, spin_limit=0):
    """Fault injection for the tests: contributors never publish their partial sums; finishers give up after spin_limit polls."""
    lib().mscnn_debug_wgemm_handoff_fault(int(bool(drop_publish)), int(spin_limit))


def debug_inner_product_rows(rows=0):
    """Rows of x per workgroup of the small-N InnerProduct kernel: 2, 4 or 8; 0 = the default (4 for N <= 5, else 2) -- tests and A/B runs."""
    lib().mscnn_debug_inner_product_rows(int(rows))
