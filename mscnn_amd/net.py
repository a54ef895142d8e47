"""ctypes binding of libmscnn_caffe.so (include/mscnn_net.h): the Caffe-compatible C++ runtime.

Mirrors the slice of matcaffe / pycaffe the reference's drivers use (caffe.Net(prototxt, 'test'), net.forward,
blob get/set; examples/kitti_car/run_mscnn_detection.m:24,72-79).  No CPU fallback."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmscnn_caffe.so")
_lib = None
_hip = None


class NetError(RuntimeError):
    pass


class DetectParams(C.Structure):
    _fields_ = [("cls_id", C.c_int), ("bbox_mean", C.c_float * 4), ("bbox_std", C.c_float * 4), ("proposal_thr", C.c_float),
                ("ratio_h", C.c_double), ("ratio_w", C.c_double), ("org_h", C.c_double), ("org_w", C.c_double),
                ("nms_overlap", C.c_double)]


class NmsParams(C.Structure):
    """mscnn_nms_params (include/mscnn_net.h): bbNms's type / ovrDnm / thr and the plain stage's det_thr."""
    _fields_ = [("type", C.c_int), ("ovr_dnm", C.c_int), ("thr", C.c_double), ("det_thr", C.c_float)]


class DetectionsView(C.Structure):
    """mscnn_detections_view (include/mscnn_net.h): where a forward's view of an image lies in the original image."""
    _fields_ = [("off_x", C.c_double), ("off_y", C.c_double), ("flip_x", C.c_int)]


class PreprocessView(C.Structure):
    """mscnn_preprocess_view (include/mscnn_net.h): window [y0, y0 + h) x [x0, x0 + w) of frame `frame`, reversed along x when flip_x."""
    _fields_ = [("frame", C.c_int), ("x0", C.c_int), ("y0", C.c_int), ("w", C.c_int), ("h", C.c_int), ("flip_x", C.c_int)]


class TrackParams(C.Structure):
    """mscnn_track_params (include/mscnn_net.h): the tracker's thresholds, motion (1 none, 2 linear), max_age and min_hits."""
    _fields_ = [("high_thr", C.c_double), ("low_thr", C.c_double), ("new_thr", C.c_double), ("match_thr", C.c_double),
                ("match_thr_low", C.c_double), ("vel_gain", C.c_double), ("motion", C.c_int), ("max_age", C.c_int), ("min_hits", C.c_int)]


class TrackKalmanParams(C.Structure):
    """mscnn_track_kalman_params (include/mscnn_net.h): the standard deviations of the per-track Kalman filter."""
    _fields_ = [("std_position", C.c_double), ("std_velocity", C.c_double), ("std_aspect", C.c_double), ("std_aspect_velocity", C.c_double),
                ("std_aspect_measure", C.c_double), ("freeze_lost_height", C.c_int)]


TRACK_KALMAN_RECORD = np.dtype([("x", "<f8", 4), ("v", "<f8", 4), ("p", "<f8", 4), ("q", "<f8", 4), ("r", "<f8", 4)])      # mscnn_track_kalman_record


class RenderParams(C.Structure):
    """mscnn_render_params (include/mscnn_net.h; 136 bytes): what the render stage draws."""
    _fields_ = [("show_thr", C.c_double), ("thickness", C.c_int), ("outline_alpha", C.c_int), ("fill_alpha", C.c_int), ("label", C.c_int),
                ("label_scale", C.c_int), ("color_by", C.c_int), ("pixelate", C.c_int), ("num_colors", C.c_int),
                ("colors", (C.c_ubyte * 3) * 32)]


class CropsParams(C.Structure):
    """mscnn_crops_params (include/mscnn_net.h; 64 bytes): which rows of the pack become patches, and how their windows are made."""
    _fields_ = [("thr", C.c_double), ("context", C.c_double), ("fit", C.c_int), ("border", C.c_int), ("min_size", C.c_int),
                ("out_h", C.c_int), ("out_w", C.c_int), ("max_crops", C.c_int), ("slot", C.c_int), ("tracked_only", C.c_int),
                ("mean_bgr", C.c_float * 3)]


class CropInfo(C.Structure):
    """mscnn_crop_info (include/mscnn_net.h; 32 bytes): where a crop came from and its window in frame pixels."""
    _fields_ = [(f, C.c_int) for f in ("frame", "slot", "row", "track_id", "x0", "y0", "w", "h")]


CROP_INFO = np.dtype([(f, "<i4") for f in ("frame", "slot", "row", "track_id", "x0", "y0", "w", "h")])
CROP_BORDERS = {"clip": 0, "shift": 1}


class CropInfoArray(np.ndarray):
    """Net.crops' second result: a CROP_INFO record array, one entry per patch, with .dropped = the rows that would have given a
    crop past max_crops (mscnn_net_crops' num_dropped)."""
    dropped = 0

    def __array_finalize__(self, obj):
        self.dropped = getattr(obj, "dropped", 0)


def crops_params(size=(128, 64), thr=0.3, context=1.0, fit=False, border="clip", min_size=1, max_crops=1, slot=None, tracked_only=False,
                 mean=(0, 0, 0)):
    """The keywords of Net.crops as a CropsParams (size = (out_h, out_w); border "clip" or "shift"; slot None = every slot)."""
    if isinstance(border, str) and border not in CROP_BORDERS:
        raise NetError(f"crops: border {border!r} is none of {sorted(CROP_BORDERS)}")
    mean = tuple(float(v) for v in mean)
    if len(mean) != 3:
        raise NetError(f"crops: mean holds {len(mean)} values (B, G, R)")
    return CropsParams(float(thr), float(context), int(fit), int(CROP_BORDERS.get(border, border)), int(min_size), int(size[0]), int(size[1]),
                       int(max_crops), -1 if slot is None else int(slot), int(tracked_only), (C.c_float * 3)(*mean))


def crop_window(params, row, org_hw):
    """mscnn_net_crop_window: the window (x0, y0, w, h) Net.crops cuts for the row [x y w h score] in a frame of org_hw = (h, w), or
    None when the row gives no crop.  params: a CropsParams, or a dict of crops_params' keywords.  Pure host code: no net, no device.
    Refused params raise NetError naming the value.  include/mscnn_net.h (mscnn_net_crops) states the rule."""
    p = params if isinstance(params, CropsParams) else crops_params(**params)
    r = (C.c_double * 5)(*[float(v) for v in row])
    win = (C.c_int * 4)()
    rc = lib().mscnn_net_crop_window(C.byref(p), r, int(org_hw[0]), int(org_hw[1]), win)
    if rc < 0:
        raise NetError(lib().mscnn_net_last_error().decode())
    return tuple(win) if rc else None


RENDER_LABELS = {"none": 0, "score": 1, "id": 2, "both": 3}
RENDER_COLOR_BY = {"slot": 0, "id": 1}
# the default palette of Net.render: eight hues that stay apart on a road scene, RGB (the look is a matter of taste no test judges)
RENDER_PALETTE = ((230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180), (70, 240, 240),
                  (240, 50, 230))

TRACK_MOTIONS = {"none": 1, "linear": 2}
TRACK_ASSIGNS = {"greedy": 1, "optimal": 2}      # MSCNN_TRACK_ASSIGN_*
TRACKS_STEPS = 5                                 # MSCNN_TRACKS_STEPS
# mscnn_track_record and a slot's header (include/mscnn_hip.h: mscnn_tracks_state_layout_of)
TRACK_RECORD = np.dtype([("box", "<f8", 4), ("obs", "<f8", 4), ("vel", "<f8", 2), ("score", "<f8"), ("id", "<i4"), ("hits", "<i4"),
                         ("misses", "<i4"), ("confirmed", "<i4")])
TRACKS_HEADER_WORDS = 8


NMS_TYPES = ("maxg", "max", "ms", "cover", "none")      # (the last three exist to be refused by name)
OVR_DNMS = ("union", "min")


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NetError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        global _hip
        _hip = C.CDLL(os.path.join(_HERE, "libmscnn_hip.so"), mode=C.RTLD_GLOBAL)
        _hip.mscnn_last_error.restype = C.c_char_p
        _hip.mscnn_nms_params_from_names.argtypes = [C.c_char_p, C.c_char_p, C.c_double, C.c_double, C.c_float, C.c_void_p]
        L = C.CDLL(LIB_PATH)
        for f in ("mscnn_net_last_error", "mscnn_net_layer_name", "mscnn_net_layer_type", "mscnn_net_layer_bottom",
                  "mscnn_net_layer_top", "mscnn_net_layer_kernel", "mscnn_net_layer_dtype", "mscnn_net_layer_param_text", "mscnn_net_blob_name", "mscnn_net_output_name"):
            getattr(L, f).restype = C.c_char_p
        L.mscnn_net_layer_flops.restype = C.c_double
        L.mscnn_net_layer_executed_flops.restype = C.c_double
        L.mscnn_net_layer_calibration_err.restype = C.c_double
        L.mscnn_net_layer_ms.restype = C.c_float
        L.mscnn_net_blob_device_ptr.restype = C.c_void_p
        L.mscnn_net_destroy.restype = None
        L.mscnn_net_detect_pack_bytes.restype = C.c_size_t
        L.mscnn_net_detect_multi_pack_bytes.restype = C.c_size_t
        L.mscnn_net_detect_cascade_multi_pack_bytes.restype = C.c_size_t
        vp, ci, cs = C.c_void_p, C.c_int, C.c_char_p
        sig = {
            "mscnn_net_create_from_file": [cs, ci, vp], "mscnn_net_create_from_string": [cs, ci, vp], "mscnn_net_destroy": [vp],
            "mscnn_net_create_from_string_ex": [cs, ci, C.c_uint, vp],
            "mscnn_net_layer_executed_flops": [vp, ci], "mscnn_net_set_conv_profiling": [vp, ci], "mscnn_net_layer_stage_ms": [vp, ci, vp],
            "mscnn_net_set_precision": [vp, cs], "mscnn_net_layer_dtype": [vp, ci],
            "mscnn_net_set_conv_algo": [vp, ci, ci], "mscnn_net_set_inner_product_algo": [vp, ci, ci], "mscnn_net_set_conv_tuning": [vp, ci, ci, ci, ci],
            "mscnn_net_calibrate_numerics": [vp, C.c_double, vp], "mscnn_net_set_numerics_watch": [vp, ci, C.c_double],
            "mscnn_net_numerics_watch_state": [vp, vp, vp, ci], "mscnn_net_layer_calibration_err": [vp, ci],
            "mscnn_net_set_auto_calibrate": [vp, C.c_double], "mscnn_net_set_chain_fusion": [vp, ci], "mscnn_net_set_boxoutput_one_pass": [vp, ci], "mscnn_net_set_roialign_one_pass": [vp, ci], "mscnn_net_roialign_pairs": [vp, vp, ci], "mscnn_net_chain_pairs": [vp, vp, vp, ci], "mscnn_net_auto_calibrate_state": [vp, vp, vp, ci],
            "mscnn_net_load_caffemodel": [vp, cs], "mscnn_net_set_stream": [vp], "mscnn_net_num_layers": [vp],
            "mscnn_net_layer_name": [vp, ci], "mscnn_net_layer_type": [vp, ci], "mscnn_net_layer_index": [vp, cs],
            "mscnn_net_layer_num_bottoms": [vp, ci], "mscnn_net_layer_num_tops": [vp, ci], "mscnn_net_layer_bottom": [vp, ci, ci],
            "mscnn_net_layer_top": [vp, ci, ci], "mscnn_net_layer_num_params": [vp, ci], "mscnn_net_layer_param_shape": [vp, ci, ci, vp, vp],
            "mscnn_net_layer_fused_away": [vp, ci], "mscnn_net_layer_param_text": [vp, ci], "mscnn_net_layer_kernel": [vp, ci], "mscnn_net_layer_flops": [vp, ci],
            "mscnn_net_num_blobs": [vp], "mscnn_net_blob_name": [vp, ci], "mscnn_net_blob_shape": [vp, cs, vp, vp],
            "mscnn_net_num_inputs": [vp], "mscnn_net_num_outputs": [vp], "mscnn_net_output_name": [vp, ci],
            "mscnn_net_set_param": [vp, ci, ci, vp, C.c_size_t], "mscnn_net_get_param": [vp, ci, ci, vp, C.c_size_t],
            "mscnn_net_set_blob": [vp, cs, vp, C.c_size_t], "mscnn_net_set_blob_device": [vp, cs, vp, C.c_size_t],
            "mscnn_net_set_image": [vp, cs, vp, ci, ci, ci, vp],
            "mscnn_net_set_images": [vp, cs, vp, ci, vp, vp, ci, vp],
            "mscnn_net_set_image_views": [vp, cs, vp, ci, vp, vp, ci, vp, ci, vp],
            "mscnn_net_get_blob": [vp, cs, vp, C.c_size_t, vp], "mscnn_net_blob_device_ptr": [vp, cs],
            "mscnn_net_forward": [vp], "mscnn_net_forward_from_to": [vp, ci, ci], "mscnn_net_reshape": [vp],
            "mscnn_net_set_layer_timing": [vp, ci], "mscnn_net_layer_ms": [vp, ci],
            "mscnn_net_set_nms": [vp, vp], "mscnn_net_get_nms": [vp, vp],
            "mscnn_net_detect": [vp, vp, vp, vp, ci, vp, vp],
            "mscnn_net_detect_cascade": [vp, vp, C.c_float, cs, cs, cs, vp, vp, ci, vp, vp],
            "mscnn_net_detect_pack_bytes": [ci], "mscnn_net_detect_device": [vp, vp, ci, vp],
            "mscnn_net_unpack_detections": [vp, ci, vp, vp, vp, vp],
            "mscnn_net_handoff_state": [vp, vp],
            "mscnn_net_detect_begin": [vp, vp, ci], "mscnn_net_detect_end": [vp, vp, vp, ci, vp, vp],
            "mscnn_net_reshape_input": [vp, cs, vp, ci], "mscnn_net_detect_image": [vp, vp, ci, vp, vp, ci, vp, vp],
            "mscnn_net_detect_multi": [vp, vp, ci, ci, vp, vp, ci, vp, vp], "mscnn_net_detect_multi_pack_bytes": [ci, ci, ci],
            "mscnn_net_detect_multi_device": [vp, vp, ci, ci, ci, vp],
            "mscnn_net_unpack_detections_multi": [vp, ci, ci, ci, vp, vp, ci, vp, vp],
            "mscnn_net_detect_cascade_multi": [vp, vp, ci, ci, ci, vp, vp, vp, C.c_float, vp, vp, ci, vp, vp],
            "mscnn_net_detect_cascade_multi_pack_bytes": [ci, ci, ci, ci],
            "mscnn_net_detect_cascade_multi_device": [vp, vp, ci, ci, ci, vp, vp, vp, C.c_float, ci, vp],
            "mscnn_net_proposals_multi": [vp, vp, ci, vp, vp, ci, vp, vp], "mscnn_net_proposals_multi_device": [vp, vp, ci, ci, vp],
            "mscnn_net_forward_proposals": [vp, vp],
            "mscnn_net_forward_rois": [vp, vp, ci, ci, ci, vp, ci, ci, vp], "mscnn_net_forward_rois_layers": [vp, vp, vp],
            "mscnn_net_detect_merge_begin": [vp, ci, ci, ci], "mscnn_net_detect_merge_add": [vp, vp, vp],
            "mscnn_net_detect_cascade_merge_add": [vp, vp, vp, ci, vp, vp, vp, C.c_float],
            "mscnn_net_detect_merge_end": [vp, vp, vp, vp, ci, vp, vp],
            "mscnn_net_detect_merge_add_views": [vp, vp, vp, vp],
            "mscnn_net_detect_cascade_merge_add_views": [vp, vp, vp, vp, ci, vp, vp, vp, C.c_float],
            "mscnn_net_set_box_voting": [vp, C.c_double], "mscnn_net_get_box_voting": [vp, vp],
            "mscnn_net_set_soft_nms": [vp, ci, C.c_double, C.c_double, ci], "mscnn_net_get_soft_nms": [vp, vp, vp, vp, vp],
            "mscnn_net_set_matrix_nms": [vp, ci, C.c_double, C.c_double, ci], "mscnn_net_get_matrix_nms": [vp, vp, vp, vp, vp],
            "mscnn_net_set_wbf": [vp, C.c_double, C.c_double, ci, ci, ci], "mscnn_net_get_wbf": [vp, vp, vp, vp, vp, vp],
            "mscnn_net_detect_merge_members": [vp, vp, ci, vp],
            "mscnn_net_set_seq_nms": [vp, C.c_double, C.c_double, ci, ci, ci], "mscnn_net_get_seq_nms": [vp, vp, vp, vp, vp, vp],
            "mscnn_net_detect_merge_sequences": [vp, vp, ci, vp],
            "mscnn_net_set_tracker": [vp, vp, ci], "mscnn_net_get_tracker": [vp, vp, vp, vp, vp], "mscnn_net_tracker_reset": [vp],
            "mscnn_net_detect_tracks": [vp, vp, ci, vp], "mscnn_net_tracker_state": [vp, vp, C.c_size_t],
            "mscnn_net_set_tracker_streams": [vp, ci], "mscnn_net_set_frame_streams": [vp, vp, ci],
            "mscnn_net_get_tracker_streams": [vp, vp, vp, ci, vp], "mscnn_net_tracker_reset_stream": [vp, ci],
            "mscnn_net_set_tracker_kalman": [vp, vp], "mscnn_net_get_tracker_kalman": [vp, vp, vp],
            "mscnn_net_tracker_kalman_state": [vp, vp, C.c_size_t],
            "mscnn_net_set_tracker_assign": [vp, C.c_int], "mscnn_net_get_tracker_assign": [vp, vp],
            "mscnn_net_render": [vp, vp, ci, vp, vp, ci, vp, vp, ci],
            "mscnn_net_crop_window": [vp, vp, ci, ci, vp], "mscnn_net_crops": [vp, vp, ci, vp, vp, ci, vp, vp, ci, vp, vp, vp],
        }
        for name, args in sig.items():
            getattr(L, name).argtypes = args
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise NetError(lib().mscnn_net_last_error().decode())


def set_stream(stream):
    """mscnn_net_set_stream: the HIP stream of every following Net call on THIS host thread -- a torch stream (anything with a
    cuda_stream attribute), a raw hipStream_t as an int, or None for the default stream.  Per thread, not per net: a net's frame
    is enqueued on the stream that is set when its calls are made; the caller orders the streams where a net changes over between
    frames, and keeps the stream alive while it is set."""
    raw = getattr(stream, "cuda_stream", stream)
    _check(lib().mscnn_net_set_stream(C.c_void_p(int(raw)) if raw else None))


class on_stream:
    """with net.on_stream(s): ... -- set_stream(s) for the block, the default stream again behind it (also when it raises)."""

    def __init__(self, stream):
        self.stream = stream

    def __enter__(self):
        set_stream(self.stream)
        return self.stream

    def __exit__(self, *exc):
        set_stream(None)
        return False


def tile_views(org_hw, rows, cols, overlap=0, flip=False, input_hw=None, frame=0):
    """The views that cut a frame of org_hw = (h, w) into rows x cols tiles which overlap by `overlap` pixels, and with flip their
    mirrors behind them.  Pure: no net, no device.  Every window has ONE size -- ceil((extent + (n - 1) * overlap) / n) per axis --,
    lies inside the frame, and together they cover it: the last row and column are shifted inwards, not shrunk.
    Returns (views, params, merge_views), one entry per view:
      views        dicts frame, x0, y0, w, h, flip_x                     for Net.set_image_views
      params       dicts org_hw = the window's size, and with input_hw   for detect_merge_add: ratios = net input / window size
                   = (H, W) of the net's input also ratios
      merge_views  dicts off_x = x0, off_y = y0, flip_x                  for detect_merge_add(..., views=, list_of=)"""
    H, W = int(org_hw[0]), int(org_hw[1])
    rows, cols, overlap = int(rows), int(cols), int(overlap)
    if H < 1 or W < 1 or rows < 1 or cols < 1 or rows > H or cols > W or overlap < 0:
        raise ValueError(f"tile_views: a {H} x {W} frame in {rows} x {cols} tiles with {overlap} pixels of overlap")
    th = -(-(H + (rows - 1) * overlap) // rows)
    tw = -(-(W + (cols - 1) * overlap) // cols)
    if th > H or tw > W or (rows > 1 and overlap >= th) or (cols > 1 and overlap >= tw):
        raise ValueError(f"tile_views: {rows} x {cols} tiles of a {H} x {W} frame with {overlap} pixels of overlap would be {th} x {tw}")
    ys = [min(r * (th - overlap), H - th) for r in range(rows)]
    xs = [min(c * (tw - overlap), W - tw) for c in range(cols)]
    views, params, merge_views = [], [], []
    for fl in ((0, 1) if flip else (0,)):
        for y0 in ys:
            for x0 in xs:
                views.append(dict(frame=frame, x0=x0, y0=y0, w=tw, h=th, flip_x=fl))
                p = dict(org_hw=(th, tw))
                if input_hw is not None:
                    p["ratios"] = (input_hw[0] / float(th), input_hw[1] / float(tw))
                params.append(p)
                merge_views.append(dict(off_x=float(x0), off_y=float(y0), flip_x=fl))
    return views, params, merge_views


class Net:
    """caffe.Net(prototxt, 'test') on one MI355X."""

    def __init__(self, prototxt_path=None, prototxt_text=None, device=0, fusion=None):
        """fusion: None = the process default (on unless MSCNN_NO_FUSE=1), True / False = explicit."""
        self._h = C.c_void_p()
        if prototxt_text is None and fusion is not None:
            prototxt_text = open(prototxt_path).read()
        if prototxt_text is not None and fusion is not None:
            _check(lib().mscnn_net_create_from_string_ex(prototxt_text.encode(), device, 0 if fusion else 1, C.byref(self._h)))
        elif prototxt_text is not None:
            _check(lib().mscnn_net_create_from_string(prototxt_text.encode(), device, C.byref(self._h)))
        else:
            _check(lib().mscnn_net_create_from_file(str(prototxt_path).encode(), device, C.byref(self._h)))
        L = lib()
        n = L.mscnn_net_num_layers(self._h)
        self.layer_names = [L.mscnn_net_layer_name(self._h, i).decode() for i in range(n)]
        self.layer_types = [L.mscnn_net_layer_type(self._h, i).decode() for i in range(n)]
        self.blob_names = [L.mscnn_net_blob_name(self._h, i).decode() for i in range(L.mscnn_net_num_blobs(self._h))]
        self.outputs = [L.mscnn_net_output_name(self._h, i).decode() for i in range(L.mscnn_net_num_outputs(self._h))]

    def __del__(self):
        try:
            if self._h:
                lib().mscnn_net_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # ---- graph ----
    def layer_bottoms(self, i):
        return [lib().mscnn_net_layer_bottom(self._h, i, k).decode() for k in range(lib().mscnn_net_layer_num_bottoms(self._h, i))]

    def layer_tops(self, i):
        return [lib().mscnn_net_layer_top(self._h, i, k).decode() for k in range(lib().mscnn_net_layer_num_tops(self._h, i))]

    def param_shapes(self, i):
        out = []
        for p in range(lib().mscnn_net_layer_num_params(self._h, i)):
            dims = (C.c_int * 8)(); nd = C.c_int()
            _check(lib().mscnn_net_layer_param_shape(self._h, i, p, dims, C.byref(nd)))
            out.append(tuple(dims[:nd.value]))
        return out

    def blob_shape(self, name):
        dims = (C.c_int * 8)(); nd = C.c_int()
        _check(lib().mscnn_net_blob_shape(self._h, name.encode(), dims, C.byref(nd)))
        return tuple(dims[:nd.value])

    def layer_param_text(self, i):
        return lib().mscnn_net_layer_param_text(self._h, i).decode()

    def fused_away(self, i):
        return bool(lib().mscnn_net_layer_fused_away(self._h, i))

    def layer_kernel(self, i):
        return lib().mscnn_net_layer_kernel(self._h, i).decode()

    def layer_flops(self, i):
        return lib().mscnn_net_layer_flops(self._h, i)

    def layer_executed_flops(self, i):
        return lib().mscnn_net_layer_executed_flops(self._h, i)

    def set_conv_profiling(self, on):
        _check(lib().mscnn_net_set_conv_profiling(self._h, int(on)))

    def layer_stage_ms(self, i):
        """(input transform, MFMA GEMM kernels, output transform) ms of layer i's last forward; zeros for non-conv layers."""
        out = (C.c_float * 3)()
        lib().mscnn_net_layer_stage_ms(self._h, i, out)
        return tuple(out)

    def set_precision(self, dtype):
        """"f32" (default, reference parity), "f16" (fp16 MFMA operands, fp32 accumulate: BASELINE config 5) or "f16x3" (the
        Winograd plane GEMMs on the fp16 pipe with exactly split operands: fp32-grade, same parity gates as "f32")."""
        _check(lib().mscnn_net_set_precision(self._h, dtype.encode()))

    def layer_dtype(self, i):
        return lib().mscnn_net_layer_dtype(self._h, i).decode()

    def set_conv_algo(self, layer, algo):
        i = layer if isinstance(layer, int) else self.layer_names.index(layer)
        _check(lib().mscnn_net_set_conv_algo(self._h, i, algo))

    def set_inner_product_algo(self, layer, algo):
        """0 = auto (fc6-class shapes on the plane-GEMM kernel), 1 = always gemm.hip's stream-K kernel; layer -1 = all."""
        i = layer if isinstance(layer, int) else self.layer_names.index(layer)
        _check(lib().mscnn_net_set_inner_product_algo(self._h, i, algo))

    def set_conv_tuning(self, layer, variant=0, grid=0, flags=0):
        i = layer if isinstance(layer, int) else self.layer_names.index(layer)
        _check(lib().mscnn_net_set_conv_tuning(self._h, i, variant, grid, flags))

    def calibrate_numerics(self, tol=5e-5):
        """After a forward on representative input: Winograd layers that stray more than tol from the direct kernel fall
        back to it.  Returns ({layer name: measured error}, [names switched])."""
        n = C.c_int()
        before = [self.layer_kernel(i) for i in range(len(self.layer_names))]
        _check(lib().mscnn_net_calibrate_numerics(self._h, tol, C.byref(n)))
        errs = {self.layer_names[i]: lib().mscnn_net_layer_calibration_err(self._h, i)
                for i in range(len(self.layer_names)) if before[i].startswith("winograd")}
        switched = [nm for nm, e in errs.items() if not e <= tol]
        assert len(switched) == n.value
        return errs, switched

    def set_auto_calibrate(self, tol=5e-5):
        """The first-forward check of every Winograd layer against the direct kernel is ON by default (5e-5); tol = 0 opts out,
        tol > 0 re-arms it with that tolerance."""
        _check(lib().mscnn_net_set_auto_calibrate(self._h, tol))

    def set_chain_fusion(self, on=True):
        """Chains of same-resolution F(4x4,3x3) convolutions keep the blob between two members out of HBM (on by default); off = every
        blob is written by every forward.  Reading such a blob re-runs its producer on demand -- same bytes either way."""
        _check(lib().mscnn_net_set_chain_fusion(self._h, int(on)))

    def set_boxoutput_one_pass(self, on=True):
        """BoxOutput of a batched net: every image side by side (on) or image after image (off, the default until the batched op has been timed) -- same bytes either way; a
        net of one image always runs the per-image op."""
        _check(lib().mscnn_net_set_boxoutput_one_pass(self._h, int(on)))

    def set_roialign_one_pass(self, on=True):
        """The ROIAlign head (two ROIAlign layers, their 2x2 AVE poolings and the Concat; the WiderFace cascade has one per stage) as one
        launch (on) or as its five layers (off, the default) -- same bytes either way, also for the grid and pooled blobs, which are
        written on demand when the head ran in one pass."""
        _check(lib().mscnn_net_set_roialign_one_pass(self._h, int(on)))

    def roialign_pairs(self):
        """[index of the first ROIAlign layer] of every head the net registered at construction."""
        a = (C.c_int * 64)()
        k = lib().mscnn_net_roialign_pairs(self._h, a, 64)
        return [a[i] for i in range(min(k, 64))]

    def chain_pairs(self):
        """[(producer layer name, consumer layer name | None)]: convolutions whose top may stay unwritten while a forward runs
        (consumer None: the top is read by its fused 2x2 pooling only)."""
        a, b = (C.c_int * 64)(), (C.c_int * 64)()
        k = lib().mscnn_net_chain_pairs(self._h, a, b, 64)
        return [(self.layer_names[a[i]], self.layer_names[b[i]] if b[i] >= 0 else None) for i in range(min(k, 64))]

    def auto_calibrate_state(self):
        """(first-forward checks done so far, [names of the layers they sent to the direct kernel], {layer: last measured error})."""
        n, sw = C.c_int(), (C.c_int * 64)()
        k = lib().mscnn_net_auto_calibrate_state(self._h, C.byref(n), sw, 64)
        errs = {nm: lib().mscnn_net_layer_calibration_err(self._h, i) for i, nm in enumerate(self.layer_names)}
        return n.value, [self.layer_names[sw[i]] for i in range(min(k, 64))], {nm: e for nm, e in errs.items() if e > 0}

    def set_numerics_watch(self, period, tol=5e-5):
        """Every period-th forward re-checks one Winograd layer (round robin) against the direct kernel on the live frame."""
        _check(lib().mscnn_net_set_numerics_watch(self._h, period, tol))

    def numerics_watch_state(self):
        """(layer checks done, [names of the layers the watch sent to the direct kernel])."""
        n, sw = C.c_int(), (C.c_int * 64)()
        k = lib().mscnn_net_numerics_watch_state(self._h, C.byref(n), sw, 64)
        return n.value, [self.layer_names[sw[i]] for i in range(min(k, 64))]

    # ---- weights ----
    def set_param(self, layer, p, arr):
        i = layer if isinstance(layer, int) else self.layer_names.index(layer)
        a = np.ascontiguousarray(arr, np.float32)
        _check(lib().mscnn_net_set_param(self._h, i, p, a.ctypes.data_as(C.c_void_p), a.size))

    def get_param(self, layer, p):
        i = layer if isinstance(layer, int) else self.layer_names.index(layer)
        shape = self.param_shapes(i)[p]
        a = np.empty(shape, np.float32)
        _check(lib().mscnn_net_get_param(self._h, i, p, a.ctypes.data_as(C.c_void_p), a.size))
        return a

    def load_caffemodel(self, path):
        _check(lib().mscnn_net_load_caffemodel(self._h, str(path).encode()))

    # ---- data ----
    def set_blob(self, name, arr):
        if hasattr(arr, "is_cuda"):   # torch CUDA tensor: device -> device
            assert arr.is_cuda and arr.is_contiguous()
            _check(lib().mscnn_net_set_blob_device(self._h, name.encode(), C.c_void_p(arr.data_ptr()), arr.numel()))
            return
        a = np.ascontiguousarray(arr, np.float32)
        _check(lib().mscnn_net_set_blob(self._h, name.encode(), a.ctypes.data_as(C.c_void_p), a.size))

    def set_image(self, name, img_rgb_u8, mean_bgr=None):
        """uint8 [H, W, 3] RGB frame (numpy array or torch CUDA tensor) -> resized / BGR / mean-subtracted input blob."""
        m = (C.c_float * 3)(*mean_bgr) if mean_bgr is not None else None
        if hasattr(img_rgb_u8, "is_cuda"):
            assert img_rgb_u8.is_cuda and img_rgb_u8.is_contiguous() and str(img_rgb_u8.dtype) == "torch.uint8"
            h, w, _ = img_rgb_u8.shape
            _check(lib().mscnn_net_set_image(self._h, name.encode(), C.c_void_p(img_rgb_u8.data_ptr()), 1, h, w, m))
            return
        a = np.ascontiguousarray(img_rgb_u8, np.uint8)
        h, w, _ = a.shape
        _check(lib().mscnn_net_set_image(self._h, name.encode(), a.ctypes.data_as(C.c_void_p), 0, h, w, m))

    def set_images(self, name, frames, mean_bgr=None):
        """Batched set_image: frames is a list of uint8 [h, w, 3] numpy arrays or a list of contiguous uint8 torch CUDA tensors (one
        frame per image of the blob, each of its own size).  Returns one dict per frame, {"ratios": (H / h, W / w), "org_hw": (h, w)}:
        the params detect_multi takes."""
        frames = list(frames)
        on_dev = [hasattr(f, "is_cuda") and f.is_cuda for f in frames]
        if any(on_dev) and not all(on_dev):
            raise NetError("set_images: a list that mixes host and device frames")
        device = any(on_dev)
        if device:
            for b, f in enumerate(frames):
                if str(f.dtype) != "torch.uint8" or f.dim() != 3 or f.shape[2] != 3 or not f.is_contiguous():
                    raise NetError(f"set_images: frame {b} is not a contiguous uint8 [h, w, 3] tensor")
            keep = frames
            ptrs = [f.data_ptr() for f in frames]
        else:
            keep = []
            for b, f in enumerate(frames):
                if not isinstance(f, np.ndarray) or f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
                    raise NetError(f"set_images: frame {b} is not a uint8 [h, w, 3] array")
                keep.append(np.ascontiguousarray(f))
            ptrs = [a.ctypes.data for a in keep]
        B = len(frames)
        hs = [int(f.shape[0]) for f in keep]
        ws = [int(f.shape[1]) for f in keep]
        m = (C.c_float * 3)(*mean_bgr) if mean_bgr is not None else None
        _check(lib().mscnn_net_set_images(self._h, name.encode(), (C.c_void_p * max(B, 1))(*ptrs), 1 if device else 0,
                                          (C.c_int * max(B, 1))(*hs), (C.c_int * max(B, 1))(*ws), B, m))
        H, W = self.blob_shape(name)[2:]
        return [{"ratios": (H / float(h), W / float(w)), "org_hw": (h, w)} for h, w in zip(hs, ws)]

    def set_image_views(self, name, frames, views, mean_bgr=None):
        """mscnn_net_set_image_views: views of one or more frames as the images of blob `name`.  frames: a list of uint8 [h, w, 3]
        numpy arrays (each uploaded once) or of contiguous uint8 torch CUDA tensors; views: one dict per image of the blob with
        frame (0), x0, y0, w, h, flip_x (0) -- tile_views makes them.  Slice v is what set_image writes for a contiguous copy of the
        window.  Returns one dict per view, {"ratios": (H / h, W / w), "org_hw": (h, w)}: the params detect_merge_add takes."""
        frames = list(frames)
        on_dev = [hasattr(f, "is_cuda") and f.is_cuda for f in frames]
        if any(on_dev) and not all(on_dev):
            raise NetError("set_image_views: a list that mixes host and device frames")
        device = any(on_dev)
        keep = []
        for b, f in enumerate(frames):
            if device:
                if str(f.dtype) != "torch.uint8" or f.dim() != 3 or f.shape[2] != 3 or not f.is_contiguous():
                    raise NetError(f"set_image_views: frame {b} is not a contiguous uint8 [h, w, 3] tensor")
                keep.append(f)
            else:
                if not isinstance(f, np.ndarray) or f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
                    raise NetError(f"set_image_views: frame {b} is not a uint8 [h, w, 3] array")
                keep.append(np.ascontiguousarray(f))
        ptrs = [f.data_ptr() for f in keep] if device else [a.ctypes.data for a in keep]
        F, V = len(keep), len(views)
        va = (PreprocessView * max(V, 1))()
        for i, v in enumerate(views):
            va[i].frame, va[i].x0, va[i].y0, va[i].w, va[i].h = int(v.get("frame", 0)), int(v["x0"]), int(v["y0"]), int(v["w"]), int(v["h"])
            va[i].flip_x = int(v.get("flip_x", 0))
        m = (C.c_float * 3)(*mean_bgr) if mean_bgr is not None else None
        _check(lib().mscnn_net_set_image_views(self._h, name.encode(), (C.c_void_p * max(F, 1))(*ptrs), 1 if device else 0,
                                               (C.c_int * max(F, 1))(*[int(f.shape[0]) for f in keep]),
                                               (C.c_int * max(F, 1))(*[int(f.shape[1]) for f in keep]), F, va, V, m))
        H, W = self.blob_shape(name)[2:]
        return [{"ratios": (H / float(va[i].h), W / float(va[i].w)), "org_hw": (va[i].h, va[i].w)} for i in range(V)]

    def get_blob(self, name):
        a = np.empty(self.blob_shape(name), np.float32)
        cnt = C.c_size_t()
        _check(lib().mscnn_net_get_blob(self._h, name.encode(), a.ctypes.data_as(C.c_void_p), a.size, C.byref(cnt)))
        return a

    def forward(self, start=0, end=-1):
        if start == 0 and end == -1:
            _check(lib().mscnn_net_forward(self._h))
        else:
            _check(lib().mscnn_net_forward_from_to(self._h, start, end))

    def forward_proposals(self):
        """mscnn_net_forward_proposals: the RPN-only run -- the layers up to the BoxOutput layer that writes proposals_score, without
        the detection sub-network.  Returns that layer's index.  proposals_multi then reads the blob as after a whole forward."""
        last = C.c_int(-1)
        _check(lib().mscnn_net_forward_proposals(self._h, C.byref(last)))
        return last.value

    def forward_rois_layers(self):
        """mscnn_net_forward_rois_layers: (L, K) -- forward_rois writes the rows into layer L's tops (the BoxOutput layer) and runs
        layers 0 .. K and L + 1 .. last."""
        L, K = C.c_int(-1), C.c_int(-1)
        _check(lib().mscnn_net_forward_rois_layers(self._h, C.byref(L), C.byref(K)))
        return L.value, K.value

    def forward_rois(self, rows, coords="net", params=None, run_trunk=True, num_images=None):
        """mscnn_net_forward_rois: the detection sub-net on caller-supplied ROIs.  rows: [R, 6] numpy array or contiguous torch CUDA
        tensor -- coords "net": float32 [image x1 y1 x2 y2 score] in net-input coordinates (the layout of proposals_score, copied bit
        for bit); coords "image": float64 [image x y w h score] in original-image pixels with a 0-based image index (the rows of
        proposals_multi) and params = one dict per image with ratios=(ratio_h, ratio_w) (the dicts set_images returns work as they
        are).  Rows grouped by image; num_images defaults to len(params), else to the input blob's N.  run_trunk=False reuses the feature blobs of the
        previous forward: the caller vouches for them.  Returns [rows per image]; detect* / proposals_multi then work as after
        forward()."""
        if coords not in ("net", "image"):
            raise NetError(f"forward_rois: coords {coords!r} ('net' or 'image')")
        code, dt, tdt = (0, np.float32, "torch.float32") if coords == "net" else (1, np.float64, "torch.float64")
        if hasattr(rows, "is_cuda"):
            if not rows.is_cuda or not rows.is_contiguous() or str(rows.dtype) != tdt or rows.dim() != 2 or rows.shape[1] != 6:
                raise NetError(f"forward_rois: rows must be a contiguous [R, 6] {tdt} CUDA tensor for coords {coords!r}")
            ptr, on_dev, R, keep = C.c_void_p(rows.data_ptr()), 1, int(rows.shape[0]), rows
        else:
            keep = np.ascontiguousarray(rows, dt)
            if keep.ndim != 2 or keep.shape[1] != 6:
                raise NetError(f"forward_rois: rows must be [R, 6], got {keep.shape}")
            ptr, on_dev, R = keep.ctypes.data_as(C.c_void_p), 0, int(keep.shape[0])
        if num_images is not None:
            N = int(num_images)
        elif params is not None:
            N = len(params)
        else:
            N = self.blob_shape(self.layer_tops(0)[0])[0]      # (the Input layer's top)
        p = None
        if params is not None:
            p = self._multi_params([{k: v for k, v in kw.items() if k == "ratios"} for kw in params], [1], org_hw=(0, 0))
        out = np.zeros(max(N, 1), np.int32)
        _check(lib().mscnn_net_forward_rois(self._h, ptr, on_dev, code, R, p, N, 1 if run_trunk else 0, out.ctypes.data_as(C.c_void_p)))
        del keep
        return out[:N].tolist()

    def reshape(self):
        _check(lib().mscnn_net_reshape(self._h))

    def reshape_input(self, name, shape):
        """net.blobs[name].reshape(*shape); net.reshape() -- another batch / frame size on the same net (Caffe order N, C, H, W)."""
        dims = (C.c_int * len(shape))(*[int(v) for v in shape])
        _check(lib().mscnn_net_reshape_input(self._h, name.encode(), dims, len(shape)))

    def handoff_state(self):
        """(stream-K hand-off time-outs this net has answered by re-running the frame, whole-tile scheduling forced for the process)."""
        forced = C.c_int()
        n = lib().mscnn_net_handoff_state(self._h, C.byref(forced))
        return n, bool(forced.value)

    def set_layer_timing(self, on):
        lib().mscnn_net_set_layer_timing(self._h, int(on))

    def layer_ms(self):
        return [lib().mscnn_net_layer_ms(self._h, i) for i in range(len(self.layer_names))]

    def set_nms(self, type="maxg", ovr_dnm="union", thr=None, det_thr=0.0, maxn=None):
        """mscnn_net_set_nms: bbNms's knobs for every detect call on this net from now on, spelled as in the reference scripts
        (pNms.type = 'maxg' | 'max', pNms.ovrDnm = 'union' | 'min'; thr None = bbNms's default -inf; det_thr: the plain stage's,
        widerface/run_mscnn_detection.m:139-143, 0 = off).  set_nms(None) restores the defaults.  'ms', 'cover', 'none', a finite
        maxn and out-of-range values are refused, naming the value; the setting then stays as it was."""
        if type is None:
            _check(lib().mscnn_net_set_nms(self._h, None))
            return
        L = lib()
        p = NmsParams()      # (the names, maxn and the ranges are checked in one place: mscnn_nms_params_from_names)
        if _hip.mscnn_nms_params_from_names(str(type).encode(), str(ovr_dnm).encode(), float("-inf") if thr is None else float(thr),
                                            float("inf") if maxn is None else float(maxn), float(det_thr), C.byref(p)) != 0:
            raise NetError("set_nms: " + _hip.mscnn_last_error().decode())
        _check(L.mscnn_net_set_nms(self._h, C.byref(p)))

    def get_nms(self):
        """mscnn_net_get_nms: the current setting as set_nms's keyword arguments (thr None = -inf)."""
        p = NmsParams()
        _check(lib().mscnn_net_get_nms(self._h, C.byref(p)))
        return dict(type=NMS_TYPES[p.type], ovr_dnm=OVR_DNMS[p.ovr_dnm], thr=None if p.thr == float("-inf") else p.thr, det_thr=p.det_thr)

    def set_box_voting(self, thr=None):
        """mscnn_net_set_box_voting: from now on detect_merge_end replaces every kept box by the prob-weighted mean of its list's
        candidates whose union overlap with it is >= thr (mscnn_detections_merge_vote_fwd).  thr None or 0 = off (the default); any
        other value must lie inside (0, 1), else the call fails naming the value and the setting stays as it was."""
        _check(lib().mscnn_net_set_box_voting(self._h, 0.0 if thr is None else float(thr)))

    def get_box_voting(self):
        """mscnn_net_get_box_voting: the current threshold, None = off."""
        thr = C.c_double()
        _check(lib().mscnn_net_get_box_voting(self._h, C.byref(thr)))
        return None if thr.value == 0.0 else thr.value

    SOFT_NMS_METHODS = {None: 0, "off": 0, "linear": 1, "gaussian": 2}

    def set_soft_nms(self, method=None, sigma=0.5, score_thr=0.001, max_out=0):
        """mscnn_net_set_soft_nms: from now on detect_merge_end runs Soft-NMS (mscnn_detections_merge_soft_fwd) in place of the hard
        NMS: a candidate that overlaps a picked box keeps living with a decayed score -- method "linear" (by 1 - IoU above nms_overlap)
        or "gaussian" (by exp(-IoU^2 / sigma)) --, picks end below score_thr or, with max_out > 0, after max_out.  method None = off
        (the default).  A refused value fails naming it and the setting stays as it was."""
        m = self.SOFT_NMS_METHODS.get(method, method) if isinstance(method, (str, type(None))) else method
        if isinstance(m, str):
            raise NetError(f"set_soft_nms: method {method!r} is none of 'linear', 'gaussian', None")
        _check(lib().mscnn_net_set_soft_nms(self._h, int(m), float(sigma), float(score_thr), int(max_out)))

    def get_soft_nms(self):
        """mscnn_net_get_soft_nms: None = off, else dict(method, sigma, score_thr, max_out)."""
        m, mo, sg, th = C.c_int(), C.c_int(), C.c_double(), C.c_double()
        _check(lib().mscnn_net_get_soft_nms(self._h, C.byref(m), C.byref(sg), C.byref(th), C.byref(mo)))
        if m.value == 0:
            return None
        return dict(method={1: "linear", 2: "gaussian"}[m.value], sigma=sg.value, score_thr=th.value, max_out=mo.value)

    def set_matrix_nms(self, method=None, sigma=0.5, score_thr=0.001, max_out=0):
        """mscnn_net_set_matrix_nms: from now on detect_merge_end runs Matrix NMS (mscnn_detections_merge_matrix_fwd) in place of the
        hard NMS: every candidate's score decayed by its worst compensated overlap with a higher-ranked one -- method "linear" or
        "gaussian" (sigma) --, no pick loop; the candidates with score' >= score_thr come back, the first max_out when max_out > 0.
        method None = off (the default).  Refused while Soft-NMS is on; a refused value fails naming it and the setting stays."""
        m = self.SOFT_NMS_METHODS.get(method, method) if isinstance(method, (str, type(None))) else method
        if isinstance(m, str):
            raise NetError(f"set_matrix_nms: method {method!r} is none of 'linear', 'gaussian', None")
        _check(lib().mscnn_net_set_matrix_nms(self._h, int(m), float(sigma), float(score_thr), int(max_out)))

    def get_matrix_nms(self):
        """mscnn_net_get_matrix_nms: None = off, else dict(method, sigma, score_thr, max_out)."""
        m, mo, sg, th = C.c_int(), C.c_int(), C.c_double(), C.c_double()
        _check(lib().mscnn_net_get_matrix_nms(self._h, C.byref(m), C.byref(sg), C.byref(th), C.byref(mo)))
        if m.value == 0:
            return None
        return dict(method={1: "linear", 2: "gaussian"}[m.value], sigma=sg.value, score_thr=th.value, max_out=mo.value)

    WBF_CONF_TYPES = {"avg": 1, "max": 2}

    def set_wbf(self, thr=None, skip_thr=0.0, conf="avg", expected=0, max_out=0):
        """mscnn_net_set_wbf: from now on detect_merge_end runs weighted boxes fusion (mscnn_detections_merge_wbf_fwd) in place of the
        hard NMS: the candidates with a score >= skip_thr are walked in score order into clusters (union overlap with the cluster's
        fused box > thr), a cluster's box is the score-weighted mean of its members, its confidence their mean (conf "avg") or largest
        ("max") score times min(members, expected) / expected; the first max_out clusters come back when max_out > 0, and
        detect_merge_members() gives their member counts.  expected 0 = the views added to the frame's lists since detect_merge_begin.
        thr None or 0 = off (the default).  Refused while Soft-NMS, Matrix NMS or box voting is on; a refused value fails naming it and
        the setting stays as it was."""
        c = self.WBF_CONF_TYPES.get(conf, conf) if isinstance(conf, str) else conf
        if isinstance(c, str):
            raise NetError(f"set_wbf: conf {conf!r} is none of 'avg', 'max'")
        _check(lib().mscnn_net_set_wbf(self._h, 0.0 if thr is None else float(thr), float(skip_thr), int(c), int(expected), int(max_out)))

    def get_wbf(self):
        """mscnn_net_get_wbf: None = off, else dict(thr, skip_thr, conf, expected, max_out)."""
        th, sk, ct, ex, mo = C.c_double(), C.c_double(), C.c_int(), C.c_int(), C.c_int()
        _check(lib().mscnn_net_get_wbf(self._h, C.byref(th), C.byref(sk), C.byref(ct), C.byref(ex), C.byref(mo)))
        if th.value == 0.0:
            return None
        return dict(thr=th.value, skip_thr=sk.value, conf={1: "avg", 2: "max"}[ct.value], expected=ex.value, max_out=mo.value)

    SEQ_NMS_RESCORES = {"avg": 1, "max": 2}

    def set_seq_nms(self, link_thr=None, score_thr=0.001, top_k=300, rescore="avg", max_out=0):
        """mscnn_net_set_seq_nms: from now on the lists of a merge are the consecutive frames of one clip and detect_merge_end runs
        Seq-NMS (mscnn_detections_merge_seq_fwd) in place of the hard NMS: per slot the boxes of neighbouring frames with a union
        overlap > link_thr are linked, the chain with the largest score sum comes out with its mean (rescore "avg") or largest ("max")
        score on every box and suppresses what its boxes overlap in their own frames, until no box is left.  Of each list the leading
        candidates with a score >= score_thr take part, at most top_k (<= 1024); the first max_out rows of a list come back when
        max_out > 0, and detect_merge_sequences() gives the sequence ids.  link_thr None or 0 = off (the default).  Refused while
        Soft-NMS, Matrix NMS or WBF is on; a refused value fails naming it and the setting stays as it was."""
        r = self.SEQ_NMS_RESCORES.get(rescore, rescore) if isinstance(rescore, str) else rescore
        if isinstance(r, str):
            raise NetError(f"set_seq_nms: rescore {rescore!r} is none of 'avg', 'max'")
        _check(lib().mscnn_net_set_seq_nms(self._h, 0.0 if link_thr is None else float(link_thr), float(score_thr), int(top_k), int(r), int(max_out)))

    def get_seq_nms(self):
        """mscnn_net_get_seq_nms: None = off, else dict(link_thr, score_thr, top_k, rescore, max_out)."""
        lt, st, tk, rs, mo = C.c_double(), C.c_double(), C.c_int(), C.c_int(), C.c_int()
        _check(lib().mscnn_net_get_seq_nms(self._h, C.byref(lt), C.byref(st), C.byref(tk), C.byref(rs), C.byref(mo)))
        if lt.value == 0.0:
            return None
        return dict(link_thr=lt.value, score_thr=st.value, top_k=tk.value, rescore={1: "avg", 2: "max"}[rs.value], max_out=mo.value)

    def set_tracker(self, high_thr=0.5, low_thr=0.1, new_thr=None, match_thr=0.3, match_thr_low=0.5, motion="linear", vel_gain=0.5,
                    max_age=30, min_hits=1, max_tracks=256, streams=1):
        """mscnn_net_set_tracker: from now on detect_multi, detect_cascade_multi and detect_merge_end step a table of tracks per slot
        behind their pack (mscnn_tracks_update_fwd: BYTE's two passes -- detections with a score >= high_thr first, overlap >
        match_thr, then those >= low_thr against the confirmed tracks seen in the frame before, overlap > match_thr_low --, motion
        "linear" = a constant-velocity prediction of the centre smoothed by vel_gain, "none" = the box stays; an unmatched detection
        >= new_thr (None: high_thr) starts a track, a track is shown once it has min_hits hits and dies after max_age missed frames),
        and detect_tracks() gives a persistent id per detection.  The images of a call, or the frames of a merge, are consecutive
        frames of the stream.  high_thr None = off (the default).  A successful call starts a fresh table (ids from 1).  Refused while
        WBF is on; a refused value fails naming it and the setting stays as it was.  While it is on the single-segment and asynchronous
        detect forms are refused.
        streams (mscnn_net_set_tracker_streams): the frames of a tracked call belong to that many streams (cameras), each with a
        table of its own; set_frame_streams says which frame is whose.  1 (the default): one stream, exactly as without.  A refused
        streams value leaves the settings as they were (the table starts afresh)."""
        if high_thr is None:
            _check(lib().mscnn_net_set_tracker(self._h, None, 0))
            return
        before = (self.get_tracker(), self.get_tracker_streams(), self.get_frame_streams()) if int(streams) != 1 else None
        m = TRACK_MOTIONS.get(motion, motion) if isinstance(motion, str) else motion
        if isinstance(m, str):
            raise NetError(f"set_tracker: motion {motion!r} is none of 'none', 'linear'")
        tp = TrackParams(float(high_thr), float(low_thr), float(high_thr if new_thr is None else new_thr), float(match_thr),
                         float(match_thr_low), float(vel_gain), int(m), int(max_age), int(min_hits))
        _check(lib().mscnn_net_set_tracker(self._h, C.byref(tp), int(max_tracks)))
        if before is not None:
            try:
                _check(lib().mscnn_net_set_tracker_streams(self._h, int(streams)))
            except NetError:
                old, old_streams, old_map = before
                if old is None:
                    self.set_tracker(None)
                else:
                    self.set_tracker(**old)
                    _check(lib().mscnn_net_set_tracker_streams(self._h, old_streams))
                    self.set_frame_streams(old_map)
                raise

    def get_tracker_streams(self):
        """mscnn_net_get_tracker_streams: the number of streams the tracker keeps tables for (1 unless set_tracker(streams=...))."""
        return self._tracker_streams()[0]

    def _tracker_streams(self):
        ns, cnt = C.c_int(), C.c_int()
        so = (C.c_int * 256)()
        _check(lib().mscnn_net_get_tracker_streams(self._h, C.byref(ns), so, 256, C.byref(cnt)))
        return ns.value, [int(so[b]) for b in range(cnt.value)]

    def set_frame_streams(self, stream_of):
        """mscnn_net_set_frame_streams: the sticky mapping for the tracked calls that follow -- image b of detect_multi and
        detect_cascade_multi, frame f of detect_merge_end, belongs to stream stream_of[b] (inside [0, streams)).  None or an empty
        sequence clears it.  With streams > 1 a tracked call needs a mapping with one entry per frame."""
        so = np.zeros(0, np.int32) if stream_of is None else np.ascontiguousarray(stream_of, dtype=np.int32).reshape(-1)
        _check(lib().mscnn_net_set_frame_streams(self._h, so.ctypes.data_as(C.c_void_p) if so.size else None, int(so.size)))

    def get_frame_streams(self):
        """The mapping set_frame_streams set (a list of ints), None when there is none."""
        return self._tracker_streams()[1] or None

    def _tracker(self):
        on, tp, mt, K = C.c_int(), TrackParams(), C.c_int(), C.c_int()
        _check(lib().mscnn_net_get_tracker(self._h, C.byref(on), C.byref(tp), C.byref(mt), C.byref(K)))
        return on.value, tp, mt.value, K.value

    def get_tracker(self):
        """mscnn_net_get_tracker: None = off, else dict(high_thr, low_thr, new_thr, match_thr, match_thr_low, motion, vel_gain, max_age,
        min_hits, max_tracks)."""
        on, tp, mt, _ = self._tracker()
        if not on:
            return None
        return dict(high_thr=tp.high_thr, low_thr=tp.low_thr, new_thr=tp.new_thr, match_thr=tp.match_thr, match_thr_low=tp.match_thr_low,
                    motion={1: "none", 2: "linear"}[tp.motion], vel_gain=tp.vel_gain, max_age=tp.max_age, min_hits=tp.min_hits, max_tracks=mt)

    def set_tracker_kalman(self, std_position=1 / 20, std_velocity=1 / 160, std_aspect=1e-2, std_aspect_velocity=1e-5,
                           std_aspect_measure=1e-1, freeze_lost_height=True):
        """mscnn_net_set_tracker_kalman: a constant-velocity Kalman filter per track on (cx, cy, w / h, h), as SORT, DeepSORT and
        ByteTrack run it, as the tracker's motion.  It needs set_tracker(motion="none") first and is refused otherwise, naming the
        motion.  std_position / std_velocity are times the track's height; freeze_lost_height: a track that missed a frame keeps its
        height.  std_position None = off (nothing changes while it is already off).  On and off start a fresh table (ids from 1) and
        keep streams and the frame mapping; set_tracker turns the filter off.  Use it where the detector's boxes jitter: it smooths
        the velocity and predicts a change of size.  On a clean, fast approaching box motion="linear" follows better."""
        if std_position is None:
            _check(lib().mscnn_net_set_tracker_kalman(self._h, None))
            return
        kp = TrackKalmanParams(float(std_position), float(std_velocity), float(std_aspect), float(std_aspect_velocity),
                               float(std_aspect_measure), int(bool(freeze_lost_height)))
        _check(lib().mscnn_net_set_tracker_kalman(self._h, C.byref(kp)))

    def get_tracker_kalman(self):
        """mscnn_net_get_tracker_kalman: None = off, else dict(std_position, std_velocity, std_aspect, std_aspect_velocity,
        std_aspect_measure, freeze_lost_height)."""
        on, kp = C.c_int(), TrackKalmanParams()
        _check(lib().mscnn_net_get_tracker_kalman(self._h, C.byref(on), C.byref(kp)))
        if not on.value:
            return None
        return dict(std_position=kp.std_position, std_velocity=kp.std_velocity, std_aspect=kp.std_aspect,
                    std_aspect_velocity=kp.std_aspect_velocity, std_aspect_measure=kp.std_aspect_measure,
                    freeze_lost_height=bool(kp.freeze_lost_height))

    def set_tracker_assign(self, method):
        """mscnn_net_set_tracker_assign: the matching of the tracker's two passes, "greedy" (the default: the walk by descending
        overlap) or "optimal" (the maximum-weight assignment SORT, DeepSORT and ByteTrack solve).  It needs the tracker on, touches
        no table -- the next tracked call goes on from the committed tracks -- and keeps streams, mapping and the Kalman filter;
        set_tracker puts it back to "greedy".  They differ where boxes overlap each other: the walk takes the best pair first and may
        leave a track with nothing that the assignment would have kept."""
        if isinstance(method, str):
            if method not in TRACK_ASSIGNS:
                raise NetError(f"set_tracker_assign: assign {method!r} is none of 'greedy', 'optimal'")
            method = TRACK_ASSIGNS[method]
        _check(lib().mscnn_net_set_tracker_assign(self._h, int(method)))

    def get_tracker_assign(self):
        """mscnn_net_get_tracker_assign: "greedy" or "optimal", None while the tracker is off."""
        m = C.c_int()
        _check(lib().mscnn_net_get_tracker_assign(self._h, C.byref(m)))
        return {1: "greedy", 2: "optimal"}.get(m.value)

    def tracker_kalman_state(self, raw=False):
        """mscnn_net_tracker_kalman_state: the committed filter table beside tracker_state()'s: per slot a numpy record array (x, v, p,
        q, r: mean, velocity, and per component the variances and the covariance) of that slot's n tracks; with streams > 1 one such
        list per stream.  raw: the table's bytes (uint8), streams * K * max_tracks records."""
        _, _, mt, K = self._tracker()
        N = self.get_tracker_streams()
        buf = np.zeros(max(N * K, 1) * mt * TRACK_KALMAN_RECORD.itemsize, np.uint8)
        _check(lib().mscnn_net_tracker_kalman_state(self._h, buf.ctypes.data_as(C.c_void_p), buf.size))
        if raw:
            return buf
        ns = [s["n"] for tab in (self.tracker_state() if N > 1 else [self.tracker_state()]) for s in tab]
        recs = buf.view(TRACK_KALMAN_RECORD).reshape(N * K, mt)
        out = [recs[k, :ns[k]].copy() for k in range(N * K)]
        return [out[s * K:(s + 1) * K] for s in range(N)] if N > 1 else out

    def tracker_reset(self, stream=None):
        """mscnn_net_tracker_reset: a new stream -- the next tracked call starts with an empty table and id 1, and fixes K again.
        stream (mscnn_net_tracker_reset_stream): only that stream's tables are reset, in front of the next tracked call's update; the
        other streams keep their tracks."""
        if stream is None:
            _check(lib().mscnn_net_tracker_reset(self._h))
        else:
            _check(lib().mscnn_net_tracker_reset_stream(self._h, int(stream)))

    def detect_tracks(self):
        """mscnn_net_detect_tracks: after a detect_multi, detect_cascade_multi or detect_merge_end that ran the tracker (set_tracker),
        the track id of every detection it returned: [[ids[D] int32 per slot] per frame], in the order of its dets; 0 = no confirmed
        track.  An error when the last of those calls ran no tracker."""
        B, K, seg = getattr(self, "_track_seg", None) or (1, 1, np.zeros(1, np.int32))
        D = int(seg.sum())
        ids = np.zeros(max(D, 1), np.int32)
        _check(lib().mscnn_net_detect_tracks(self._h, ids.ctypes.data_as(C.c_void_p), D, seg.ctypes.data_as(C.c_void_p)))
        ends = np.cumsum(seg)
        return [[ids[ends[i * K + k] - seg[i * K + k]:ends[i * K + k]].copy() for k in range(K)] for i in range(B)]

    def render(self, frames, thr=0.3, thickness=2, label="score", color_by="slot", pixelate=0, outline_alpha=256, fill_alpha=0,
               label_scale=1, colors=RENDER_PALETTE, out=None):
        """mscnn_net_render: the detections of the last detect_multi, detect_cascade_multi or detect_merge_end -- and its track ids, if
        it ran the tracker -- drawn into copies of the frames it detected on: every box with score >= thr outlined (thickness pixels,
        blended with outline_alpha of 256), filled with fill_alpha, labelled ("none", "score", "id", "both") in glyphs magnified
        label_scale times, coloured by "slot" or by track "id" from colors (1 .. 32 RGB triples); pixelate = N replaces every box's
        interior with an N x N mosaic of the source.  frames: uint8 [h, w, 3] numpy arrays, or contiguous uint8 CUDA tensors (then
        nothing but the pack crosses the bus and the result is a list of CUDA tensors: out, or new ones); otherwise a list of numpy
        arrays.  include/mscnn_hip.h (mscnn_render_detections_u8) states the pixels."""
        for name, table, v in (("label", RENDER_LABELS, label), ("color_by", RENDER_COLOR_BY, color_by)):
            if isinstance(v, str) and v not in table:
                raise NetError(f"render: {name} {v!r} is none of {sorted(table)}")
        cols = [tuple(int(v) for v in c) for c in colors]
        if len(cols) > 32 or any(len(c) != 3 or min(c) < 0 or max(c) > 255 for c in cols):
            raise NetError(f"render: colors holds {len(cols)} entries (at most 32 RGB triples of 0 .. 255)")
        p = RenderParams(float(thr), int(thickness), int(outline_alpha), int(fill_alpha), int(RENDER_LABELS.get(label, label)),
                         int(label_scale), int(RENDER_COLOR_BY.get(color_by, color_by)), int(pixelate), len(cols))
        for i, c in enumerate(cols):
            p.colors[i][:] = c
        frames = list(frames)
        on_dev = [hasattr(f, "is_cuda") and f.is_cuda for f in frames]
        if any(on_dev) and not all(on_dev):
            raise NetError("render: a list that mixes host and device frames")
        device = any(on_dev)
        if device:
            import torch
            for b, f in enumerate(frames):
                if str(f.dtype) != "torch.uint8" or f.dim() != 3 or f.shape[2] != 3 or not f.is_contiguous():
                    raise NetError(f"render: frame {b} is not a contiguous uint8 [h, w, 3] tensor")
            keep = frames
            outs = [torch.empty_like(f) for f in frames] if out is None else list(out)
            if len(outs) != len(frames) or any(o.shape != f.shape or o.dtype != f.dtype or not o.is_cuda or not o.is_contiguous()
                                               for o, f in zip(outs, frames)):
                raise NetError("render: out does not hold one contiguous uint8 CUDA tensor of each frame's shape")
            ptrs, optrs = [f.data_ptr() for f in frames], [o.data_ptr() for o in outs]
        else:
            keep = []
            for b, f in enumerate(frames):
                if not isinstance(f, np.ndarray) or f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
                    raise NetError(f"render: frame {b} is not a uint8 [h, w, 3] array")
                keep.append(np.ascontiguousarray(f))
            outs = [np.empty_like(a) for a in keep]
            ptrs, optrs = [a.ctypes.data for a in keep], [o.ctypes.data for o in outs]
        B = len(frames)
        hs = [int(f.shape[0]) for f in keep]
        ws = [int(f.shape[1]) for f in keep]
        _check(lib().mscnn_net_render(self._h, (C.c_void_p * max(B, 1))(*ptrs), 1 if device else 0, (C.c_int * max(B, 1))(*hs),
                                      (C.c_int * max(B, 1))(*ws), B, C.byref(p), (C.c_void_p * max(B, 1))(*optrs), 1 if device else 0))
        return outs

    def crops(self, frames, size=(128, 64), thr=0.3, context=1.0, fit=False, border="clip", min_size=1, max_crops=None, slot=None,
              tracked_only=False, mean=(0, 0, 0), out=None):
        """mscnn_net_crops: every detection of the last detect_multi, detect_cascade_multi or detect_merge_end with score >= thr as a
        float32 patch of size = (out_h, out_w), planes B, G, R with mean subtracted, cut out of the frames it detected on and resized on
        the device (the scripts' imresize).  The window is the box scaled about its centre by context (1 .. 16), with fit grown to the
        patch's aspect ratio, then clipped to the frame (border "clip") or moved inwards ("shift"); windows under min_size pixels give
        no crop; slot = only that slot; tracked_only = only rows with a track id > 0 (needs set_tracker).  include/mscnn_net.h states
        the window rule, crop_window() computes it for one row.
        Returns (patches, info).  patches: [n, 3, out_h, out_w] -- a numpy array for host frames (uint8 [h, w, 3] arrays), a CUDA
        tensor for contiguous uint8 CUDA tensors (then only the windows' table crosses the bus, and the call is asynchronous on the
        net's stream).  out: a contiguous float32 buffer [>= max_crops, 3, out_h, out_w] to write into, numpy or CUDA whatever the
        frames are; patches is then out[:n], and the slices behind it are untouched.  info: a CropInfoArray (records frame, slot, row,
        track_id, x0, y0, w, h; row = the index in its segment), in the order (frame, slot, row); info.dropped = the rows that would
        have given a crop past max_crops.  max_crops None: out's first dimension, else the number of rows that call returned, so that
        nothing can be dropped.  Like render it reads the pack and steps nothing; both may follow one detect call in either order."""
        frames = list(frames)
        on_dev = [hasattr(f, "is_cuda") and f.is_cuda for f in frames]
        if any(on_dev) and not all(on_dev):
            raise NetError("crops: a list that mixes host and device frames")
        device = any(on_dev)
        if device:
            for b, f in enumerate(frames):
                if str(f.dtype) != "torch.uint8" or f.dim() != 3 or f.shape[2] != 3 or not f.is_contiguous():
                    raise NetError(f"crops: frame {b} is not a contiguous uint8 [h, w, 3] tensor")
            keep = frames
            ptrs = [f.data_ptr() for f in frames]
        else:
            keep = []
            for b, f in enumerate(frames):
                if not isinstance(f, np.ndarray) or f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
                    raise NetError(f"crops: frame {b} is not a uint8 [h, w, 3] array")
                keep.append(np.ascontiguousarray(f))
            ptrs = [a.ctypes.data for a in keep]
        oh, ow = int(size[0]), int(size[1])
        if max_crops is None:
            seg = getattr(self, "_track_seg", None)
            max_crops = int(out.shape[0]) if out is not None else max(1, int(seg[2].sum()) if seg else 1)
        p = crops_params((oh, ow), thr, context, fit, border, min_size, max_crops, slot, tracked_only, mean)
        rows = max(int(max_crops), 1)
        out_dev = device if out is None else bool(getattr(out, "is_cuda", False))
        if out is None:
            if 1 <= oh <= 1024 and 1 <= ow <= 1024:
                shape = (rows, 3, oh, ow)
            else:
                shape = (1, 3, 1, 1)      # (the call refuses the size, naming it)
            if out_dev:
                import torch
                buf = torch.empty(shape, dtype=torch.float32, device=frames[0].device)
            else:
                buf = np.empty(shape, np.float32)
        else:
            buf = out
            ok = (tuple(buf.shape[1:]) == (3, oh, ow) and buf.shape[0] >= rows and (
                (str(buf.dtype) == "torch.float32" and buf.is_contiguous()) if out_dev else
                (isinstance(buf, np.ndarray) and buf.dtype == np.float32 and buf.flags.c_contiguous)))
            if not ok:
                raise NetError(f"crops: out is not a contiguous float32 buffer of shape [>= {rows}, 3, {oh}, {ow}]")
        info = np.zeros(rows, CROP_INFO)
        n, dropped = C.c_int(0), C.c_int(0)
        B = len(frames)
        hs = [int(f.shape[0]) for f in keep]
        ws = [int(f.shape[1]) for f in keep]
        _check(lib().mscnn_net_crops(self._h, (C.c_void_p * max(B, 1))(*ptrs), 1 if device else 0, (C.c_int * max(B, 1))(*hs),
                                     (C.c_int * max(B, 1))(*ws), B, C.byref(p), C.c_void_p(buf.data_ptr() if out_dev else buf.ctypes.data),
                                     1 if out_dev else 0, info.ctypes.data_as(C.c_void_p), C.byref(n), C.byref(dropped)))
        res = info[:n.value].view(CropInfoArray)
        res.dropped = dropped.value
        return buf[:n.value], res

    def tracker_state(self, raw=False):
        """mscnn_net_tracker_state: the committed table, one dict per slot -- n, next_id, frame, dropped, skipped and tracks = the
        first n records (a numpy record array: box, obs, vel, score, id, hits, misses, confirmed).  Under set_tracker_assign("optimal")
        only, also steps = the table's running total of search steps (header word 5).  With streams > 1 one such list
        per stream.  raw: the table's bytes (uint8), streams * K slots, (stream s, slot k) at s * K + k."""
        _, _, mt, K = self._tracker()
        N = self.get_tracker_streams()
        per_stream, K = K, N * K
        slot = 4 * TRACKS_HEADER_WORDS + mt * TRACK_RECORD.itemsize
        buf = np.zeros((max(K, 1) * slot + 15) // 16 * 16, np.uint8)
        _check(lib().mscnn_net_tracker_state(self._h, buf.ctypes.data_as(C.c_void_p), buf.size))
        if raw:
            return buf
        out = []
        optimal = self.get_tracker_assign() == "optimal"
        for k in range(K):
            h = buf[k * slot:k * slot + 4 * TRACKS_HEADER_WORDS].view(np.int32)
            at = k * slot + 4 * TRACKS_HEADER_WORDS
            recs = buf[at:at + int(h[0]) * TRACK_RECORD.itemsize].view(TRACK_RECORD).copy()
            out.append(dict(n=int(h[0]), next_id=int(h[1]), frame=int(h[2]), dropped=int(h[3]), skipped=int(h[4]), tracks=recs))
            if optimal:
                out[-1]["steps"] = int(h[TRACKS_STEPS])
        if N > 1:
            return [out[s * per_stream:(s + 1) * per_stream] for s in range(N)]
        return out

    @staticmethod
    def _params(cls_id, ratios, org_hw, bbox_mean, bbox_std, proposal_thr, nms_overlap):
        p = DetectParams()
        p.cls_id = cls_id
        for k in range(4):
            p.bbox_mean[k] = bbox_mean[k]; p.bbox_std[k] = bbox_std[k]
        p.proposal_thr = proposal_thr
        p.ratio_h, p.ratio_w = ratios
        p.org_h, p.org_w = org_hw
        p.nms_overlap = nms_overlap
        return p

    def detect_device(self, cap, cls_id, ratios, org_hw, bbox_mean=(0, 0, 0, 0), bbox_std=(0.1, 0.1, 0.2, 0.2),
                      proposal_thr=-10.0, nms_overlap=0.5):
        """Final stage into the fixed-capacity DEVICE pack (multi-GPU gather input, include/mscnn_dist.h); asynchronous.
        Returns the device address of the pack (detect_pack_bytes(cap) bytes)."""
        p = self._params(cls_id, ratios, org_hw, bbox_mean, bbox_std, proposal_thr, nms_overlap)
        ptr = C.c_void_p()
        _check(lib().mscnn_net_detect_device(self._h, C.byref(p), cap, C.byref(ptr)))
        return ptr.value

    def detect_begin(self, cap, cls_id, ratios, org_hw, bbox_mean=(0, 0, 0, 0), bbox_std=(0.1, 0.1, 0.2, 0.2), proposal_thr=-10.0,
                     nms_overlap=0.5):
        """mscnn_net_detect_begin: final stage of the forward just done + an asynchronous copy of its pack to pinned host memory; go
        on with the next frame and collect with detect_end (at most two frames in flight)."""
        p = self._params(cls_id, ratios, org_hw, bbox_mean, bbox_std, proposal_thr, nms_overlap)
        _check(lib().mscnn_net_detect_begin(self._h, C.byref(p), cap))

    def detect_end(self, cap):
        """mscnn_net_detect_end: (dets [D, 5] float64, ids [D] int32, R) of the oldest frame in flight."""
        rows = max(cap, 1)
        if getattr(self, "_end_rows", 0) != rows:
            self._end_dets = np.zeros((rows, 5), np.float64); self._end_ids = np.zeros(rows, np.int32); self._end_rows = rows
        D = C.c_int(); R = C.c_int()
        _check(lib().mscnn_net_detect_end(self._h, self._end_dets.ctypes.data_as(C.c_void_p), self._end_ids.ctypes.data_as(C.c_void_p), cap,
                                          C.byref(D), C.byref(R)))
        return self._end_dets[:D.value].copy(), self._end_ids[:D.value].copy(), R.value

    def detect_cascade(self, bbox_blob, prob_blob, proposal_blob, cls_id, ratios, org_hw, det_thr=0.0, nms_overlap=0.5, cap=4096):
        """Final stage of the cascade drivers (run_cascademscnn.m:84-127) for one cascade output; returns (dets, ids, R)."""
        p = self._params(cls_id, ratios, org_hw, (0, 0, 0, 0), (1, 1, 1, 1), 0.0, nms_overlap)
        dets = np.zeros((cap, 5), np.float64); ids = np.zeros(cap, np.int32)
        D = C.c_int(); R = C.c_int()
        _check(lib().mscnn_net_detect_cascade(self._h, C.byref(p), det_thr, bbox_blob.encode(), prob_blob.encode(), proposal_blob.encode(),
                                              dets.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p), cap, C.byref(D), C.byref(R)))
        return dets[:D.value].copy(), ids[:D.value].copy(), R.value

    @classmethod
    def _multi_params(cls, params, classes, num_outputs=1, **defaults):
        """params: one dict per image (ratios, org_hw; optional bbox_mean, bbox_std, proposal_thr, nms_overlap), classes: cls_ids
        -> the (image, output, class) parameter array of mscnn_net_detect_multi / _cascade_multi, image-major."""
        defaults = dict(dict(bbox_mean=(0, 0, 0, 0), bbox_std=(0.1, 0.1, 0.2, 0.2), proposal_thr=-10.0, nms_overlap=0.5), **defaults)
        K = num_outputs * len(classes)
        arr = (DetectParams * max(len(params) * K, 1))()
        for i, kw in enumerate(params):
            kw = dict(defaults, **kw)
            for k in range(K):
                arr[i * K + k] = cls._params(classes[k % len(classes)], **kw)
        return arr

    @classmethod
    def _cascade_multi_args(cls, params, outputs, classes):
        """-> (the (image, output, class) parameter array, the three blob name arrays) of mscnn_net_detect_cascade_multi."""
        O = len(outputs)
        keep = ("ratios", "org_hw", "nms_overlap")
        arr = cls._multi_params([{k: v for k, v in kw.items() if k in keep} for kw in params], classes, O, bbox_std=(1, 1, 1, 1), proposal_thr=0.0)
        names = [(C.c_char_p * max(O, 1))(*[None if t[k] is None else t[k].encode() for t in outputs]) for k in range(3)]
        return arr, names

    def detect_cascade_multi(self, params, outputs, classes, det_thr=0.0, cap=None):
        """mscnn_net_detect_cascade_multi: the cascade final stage (run_cascademscnn.m:84-127) of every image, cascade output and
        class of the last forward in one pass.  params: one dict per image of the batch (ratios, org_hw, optionally nms_overlap --
        the dicts set_images returns work as they are); outputs: [(bbox_blob, prob_blob, proposal_blob)] per cascade output;
        classes: the cls_ids.  Returns (per_image[i][o][c] = (dets[D,5], rows of the net's blobs[D]), [ROI count per image])."""
        B, O, Cn = len(params), len(outputs), len(classes)
        if cap is None:
            cap = max(1, O * Cn * self.blob_shape(outputs[0][0])[0]) if O and outputs[0][0] in self.blob_names else 1
        p, (bb, pb, qb) = self._cascade_multi_args(params, outputs, classes)
        dets = np.zeros((max(cap, 1), 5), np.float64); ids = np.zeros(max(cap, 1), np.int32)
        seg = np.zeros(max(B * O * Cn, 1), np.int32); rois = np.zeros(max(B, 1), np.int32)
        _check(lib().mscnn_net_detect_cascade_multi(self._h, p, B, O, Cn, bb, pb, qb, det_thr, dets.ctypes.data_as(C.c_void_p),
                                                    ids.ctypes.data_as(C.c_void_p), cap, seg.ctypes.data_as(C.c_void_p),
                                                    rois.ctypes.data_as(C.c_void_p)))
        self._track_seg = (B, O * Cn, seg[:B * O * Cn].copy())
        flat = _split_segments(dets, ids, seg, B, O * Cn)
        return [[row[o * Cn:(o + 1) * Cn] for o in range(O)] for row in flat], rois[:B].tolist()

    def detect_cascade_multi_device(self, params, outputs, classes, cap, det_thr=0.0):
        """mscnn_net_detect_cascade_multi_device: the same into the device pack (detect_cascade_multi_pack_bytes(B, O, C, cap)
        bytes); asynchronous.  Returns its device address; unpack_detections_cascade_multi reads a host copy of it."""
        p, (bb, pb, qb) = self._cascade_multi_args(params, outputs, classes)
        ptr = C.c_void_p()
        _check(lib().mscnn_net_detect_cascade_multi_device(self._h, p, len(params), len(outputs), len(classes), bb, pb, qb, det_thr, cap,
                                                           C.byref(ptr)))
        return ptr.value

    def detect_image(self, image, cls_id, ratios, org_hw, bbox_mean=(0, 0, 0, 0), bbox_std=(0.1, 0.1, 0.2, 0.2), proposal_thr=-10.0,
                     nms_overlap=0.5, cap=4096):
        """The final stage for image `image` of a batched forward; returns (dets[D,5], rows of the net's ROI blobs[D], the image's R)."""
        p = self._params(cls_id, ratios, org_hw, bbox_mean, bbox_std, proposal_thr, nms_overlap)
        dets = np.zeros((cap, 5), np.float64); ids = np.zeros(cap, np.int32)
        D = C.c_int(); R = C.c_int()
        _check(lib().mscnn_net_detect_image(self._h, C.byref(p), image, dets.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p), cap,
                                            C.byref(D), C.byref(R)))
        return dets[:D.value].copy(), ids[:D.value].copy(), R.value

    def detect_multi(self, params, classes, cap=None):
        """mscnn_net_detect_multi: the final stage of every image and class of the last forward in one pass.  params: one dict per
        image of the batch (ratios, org_hw, optionally bbox_mean / bbox_std / proposal_thr / nms_overlap); classes: the cls_ids.
        Returns ([[(dets[D,5], rows of the net's ROI blobs[D]) per class] per image], [ROI count per image]) -- each pair equal to
        detect_image(image, cls_id, ...)."""
        B, Cn = len(params), len(classes)
        if cap is None:
            cap = max(1, Cn * self.blob_shape("proposals_score")[0])
        p = self._multi_params(params, classes)
        dets = np.zeros((max(cap, 1), 5), np.float64); ids = np.zeros(max(cap, 1), np.int32)
        seg = np.zeros(B * Cn, np.int32); rois = np.zeros(B, np.int32)
        _check(lib().mscnn_net_detect_multi(self._h, p, B, Cn, dets.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p), cap,
                                            seg.ctypes.data_as(C.c_void_p), rois.ctypes.data_as(C.c_void_p)))
        self._track_seg = (B, Cn, seg.copy())
        return _split_segments(dets, ids, seg, B, Cn), rois.tolist()

    # ---- several forwards of a frame, one NMS (mscnn_net_detect_merge_*)
    @staticmethod
    def _views(views, B):
        """views: None (the identity), or one dict per image with off_x / off_y / flip_x (missing: 0) -> the view array or None."""
        if views is None:
            return None
        if len(views) != B:
            raise NetError(f"detect_merge: {len(views)} views for {B} images")
        arr = (DetectionsView * max(B, 1))()
        for i, v in enumerate(views):
            arr[i].off_x, arr[i].off_y, arr[i].flip_x = float(v.get("off_x", 0.0)), float(v.get("off_y", 0.0)), int(v.get("flip_x", 0))
        return arr

    def detect_merge_begin(self, num_images, num_classes, cand_cap):
        """mscnn_net_detect_merge_begin: reserve and reset num_images x num_classes candidate lists of cand_cap slots (for the cascade
        form num_classes = outputs x classes).  Then, per forward, detect_merge_add / detect_cascade_merge_add, and detect_merge_end."""
        _check(lib().mscnn_net_detect_merge_begin(self._h, num_images, num_classes, cand_cap))
        self._merge_shape = (num_images, num_classes, cand_cap)

    def detect_merge_add(self, params, classes, views=None, *, list_of=None):
        """mscnn_net_detect_merge_add after a forward.  params: one dict per image as in detect_multi, describing THIS forward's view
        (ratios = input size / view size, org_hw = the view's size); views: None or one dict per image (off_x, off_y, flip_x).
        list_of (keyword only): mscnn_net_detect_merge_add_views -- the input's images are views of the merge's frames, image b goes to
        the lists of frame list_of[b]; one call is one pass, a list's order (add call, image, row)."""
        p = self._multi_params(params, classes)
        if list_of is None:
            _check(lib().mscnn_net_detect_merge_add(self._h, p, self._views(views, len(params))))
            return
        _check(lib().mscnn_net_detect_merge_add_views(self._h, p, self._views(views, len(params)), self._list_of(list_of, len(params))))

    @staticmethod
    def _list_of(list_of, B):
        if len(list_of) != B:
            raise NetError(f"detect_merge: {len(list_of)} list_of entries for {B} images")
        return (C.c_int * max(B, 1))(*[int(v) for v in list_of])

    def detect_cascade_merge_add(self, params, outputs, classes, det_thr=0.0, views=None, *, list_of=None):
        """mscnn_net_detect_cascade_merge_add: the same for a cascade deploy; outputs, classes, det_thr as in detect_cascade_multi.
        list_of (keyword only): mscnn_net_detect_cascade_merge_add_views, as in detect_merge_add."""
        p, (bb, pb, qb) = self._cascade_multi_args(params, outputs, classes)
        if list_of is None:
            _check(lib().mscnn_net_detect_cascade_merge_add(self._h, p, self._views(views, len(params)), len(outputs), bb, pb, qb, det_thr))
            return
        _check(lib().mscnn_net_detect_cascade_merge_add_views(self._h, p, self._views(views, len(params)), self._list_of(list_of, len(params)),
                                                              len(outputs), bb, pb, qb, det_thr))

    def detect_merge_end(self, cap=None):
        """mscnn_net_detect_merge_end: one NMS over each list.  Returns ([[(dets[D,5], pass[D], row[D]) per slot] per image],
        [[candidates per slot] per image]); pass = the add (0-based) a detection came from, row = the row of that forward's ROI
        blobs.  cap: rows of the host buffers (default: every candidate slot)."""
        shape = getattr(self, "_merge_shape", None)
        B, K, cand_cap = shape if shape else (1, 1, 1)
        self._merge_shape = None
        S = B * K
        if cap is None:
            cap = S * cand_cap
        dets = np.zeros((max(cap, 1), 5), np.float64)
        pas = np.zeros(max(cap, 1), np.int32); row = np.zeros(max(cap, 1), np.int32)
        seg = np.zeros(S, np.int32); cands = np.zeros(S, np.int32)
        vp = C.c_void_p
        _check(lib().mscnn_net_detect_merge_end(self._h, dets.ctypes.data_as(vp), pas.ctypes.data_as(vp), row.ctypes.data_as(vp), cap,
                                                seg.ctypes.data_as(vp), cands.ctypes.data_as(vp)))
        self._merge_seg = (B, K, seg.copy())
        self._track_seg = self._merge_seg
        out, o = [], 0
        for i in range(B):
            per = []
            for k in range(K):
                d = int(seg[i * K + k])
                per.append((dets[o:o + d].copy(), pas[o:o + d].copy(), row[o:o + d].copy()))
                o += d
            out.append(per)
        return out, cands.reshape(B, K).tolist()

    def detect_merge_members(self):
        """mscnn_net_detect_merge_members: after a detect_merge_end that ran weighted boxes fusion (set_wbf), the member count of every
        detection it returned: [[members[D] int32 per slot] per image], in the order of its dets.  An error when it ran no WBF."""
        B, K, seg = getattr(self, "_merge_seg", None) or (1, 1, np.zeros(1, np.int32))
        D = int(seg.sum())
        mem = np.zeros(max(D, 1), np.int32)
        _check(lib().mscnn_net_detect_merge_members(self._h, mem.ctypes.data_as(C.c_void_p), D, seg.ctypes.data_as(C.c_void_p)))
        ends = np.cumsum(seg)
        return [[mem[ends[i * K + k] - seg[i * K + k]:ends[i * K + k]].copy() for k in range(K)] for i in range(B)]

    def detect_merge_sequences(self):
        """mscnn_net_detect_merge_sequences: after a detect_merge_end that ran Seq-NMS (set_seq_nms), the sequence id of every detection
        it returned: [[seq[D] int32 per slot] per frame], in the order of its dets; an id is unique within the clip and slot.  An error
        when it ran no Seq-NMS."""
        B, K, seg = getattr(self, "_merge_seg", None) or (1, 1, np.zeros(1, np.int32))
        D = int(seg.sum())
        ids = np.zeros(max(D, 1), np.int32)
        _check(lib().mscnn_net_detect_merge_sequences(self._h, ids.ctypes.data_as(C.c_void_p), D, seg.ctypes.data_as(C.c_void_p)))
        ends = np.cumsum(seg)
        return [[ids[ends[i * K + k] - seg[i * K + k]:ends[i * K + k]].copy() for k in range(K)] for i in range(B)]

    def detect_multi_device(self, params, classes, cap):
        """mscnn_net_detect_multi_device: the same into the device pack (detect_multi_pack_bytes(B, C, cap) bytes); asynchronous.
        Returns its device address."""
        p = self._multi_params(params, classes)
        ptr = C.c_void_p()
        _check(lib().mscnn_net_detect_multi_device(self._h, p, len(params), len(classes), cap, C.byref(ptr)))
        return ptr.value

    def proposals_multi(self, params, cap=None):
        """mscnn_net_proposals_multi: the proposal half of the scripts' result (run_mscnn_detection.m:75-91, final_proposals{k}) of
        every image of the last forward in one pass.  params: one dict per image of the batch (ratios, optionally proposal_thr; the
        dicts set_images returns work as they are).  Returns ([(props [n, 5] float64 [x y w h score], rows [n] int32 = rows of the
        net's ROI blobs, the convention of detect_multi's ids) per image], [ROI count per image])."""
        B = len(params)
        if cap is None:
            cap = max(1, self.blob_shape("proposals_score")[0]) if "proposals_score" in self.blob_names else 1
        p = self._multi_params([{k: v for k, v in kw.items() if k in ("ratios", "proposal_thr")} for kw in params], [1], org_hw=(0, 0))
        props = np.zeros((max(cap, 1), 5), np.float64); rows = np.zeros(max(cap, 1), np.int32)
        cnt = np.zeros(max(B, 1), np.int32); rois = np.zeros(max(B, 1), np.int32)
        _check(lib().mscnn_net_proposals_multi(self._h, p, B, props.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p), cap,
                                               cnt.ctypes.data_as(C.c_void_p), rois.ctypes.data_as(C.c_void_p)))
        return [seg[0] for seg in _split_segments(props, rows, cnt, B, 1)], rois[:B].tolist()

    def proposals_multi_device(self, params, cap):
        """mscnn_net_proposals_multi_device: the same into the device pack (detect_multi_pack_bytes(B, 1, cap) bytes); asynchronous.
        Returns its device address; unpack_detections_multi(pack, B, 1, cap) reads a host copy of it."""
        p = self._multi_params([{k: v for k, v in kw.items() if k in ("ratios", "proposal_thr")} for kw in params], [1], org_hw=(0, 0))
        ptr = C.c_void_p()
        _check(lib().mscnn_net_proposals_multi_device(self._h, p, len(params), cap, C.byref(ptr)))
        return ptr.value

    def detect(self, cls_id, ratios, org_hw, bbox_mean=(0, 0, 0, 0), bbox_std=(0.1, 0.1, 0.2, 0.2), proposal_thr=-10.0,
               nms_overlap=0.5, cap=4096):
        """Final detection stage on the device; returns (dets[D,5] float64 [x y w h prob], roi ids[D], R)."""
        p = self._params(cls_id, ratios, org_hw, bbox_mean, bbox_std, proposal_thr, nms_overlap)
        dets = np.zeros((cap, 5), np.float64); ids = np.zeros(cap, np.int32)
        D = C.c_int(); R = C.c_int()
        _check(lib().mscnn_net_detect(self._h, C.byref(p), dets.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p), cap,
                                      C.byref(D), C.byref(R)))
        return dets[:D.value].copy(), ids[:D.value].copy(), R.value


def detect_pack_bytes(cap):
    return lib().mscnn_net_detect_pack_bytes(cap)


def unpack_detections(pack_host, cap):
    """One host copy of a detection pack (bytes / ctypes buffer / numpy uint8) -> (dets[D,5] float64, ids[D] int32, R)."""
    buf = np.frombuffer(pack_host, np.uint8) if not isinstance(pack_host, np.ndarray) else pack_host
    assert buf.nbytes >= detect_pack_bytes(cap)
    buf = np.ascontiguousarray(buf)
    dets = np.zeros((max(cap, 1), 5), np.float64); ids = np.zeros(max(cap, 1), np.int32)
    D = C.c_int(); R = C.c_int()
    _check(lib().mscnn_net_unpack_detections(buf.ctypes.data_as(C.c_void_p), cap, dets.ctypes.data_as(C.c_void_p),
                                             ids.ctypes.data_as(C.c_void_p), C.byref(D), C.byref(R)))
    return dets[:D.value].copy(), ids[:D.value].copy(), R.value


def detect_multi_pack_bytes(num_images, num_classes, cap):
    return lib().mscnn_net_detect_multi_pack_bytes(num_images, num_classes, cap)


def _split_segments(dets, ids, seg, B, Cn):
    out, o = [], 0
    for i in range(B):
        row = []
        for c in range(Cn):
            k = int(seg[i * Cn + c])
            row.append((dets[o:o + k].copy(), ids[o:o + k].copy()))
            o += k
        out.append(row)
    return out


def unpack_detections_multi(pack_host, num_images, num_classes, cap, out_cap=None):
    """One host copy of a multi pack (mscnn_net_detect_multi_device) -> ([[(dets, ids)] per class] per image, [ROI count per image])."""
    buf = np.frombuffer(pack_host, np.uint8) if not isinstance(pack_host, np.ndarray) else pack_host
    assert buf.nbytes >= detect_multi_pack_bytes(num_images, num_classes, cap)
    buf = np.ascontiguousarray(buf)
    out_cap = max(cap, 1) if out_cap is None else out_cap
    dets = np.zeros((max(out_cap, 1), 5), np.float64); ids = np.zeros(max(out_cap, 1), np.int32)
    seg = np.zeros(num_images * num_classes, np.int32); rois = np.zeros(num_images, np.int32)
    _check(lib().mscnn_net_unpack_detections_multi(buf.ctypes.data_as(C.c_void_p), num_images, num_classes, cap,
                                                   dets.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p), out_cap,
                                                   seg.ctypes.data_as(C.c_void_p), rois.ctypes.data_as(C.c_void_p)))
    return _split_segments(dets, ids, seg, num_images, num_classes), rois.tolist()


def detect_cascade_multi_pack_bytes(num_images, num_outputs, num_classes, cap):
    return lib().mscnn_net_detect_cascade_multi_pack_bytes(num_images, num_outputs, num_classes, cap)


def unpack_detections_cascade_multi(pack_host, num_images, num_outputs, num_classes, cap, out_cap=None):
    """One host copy of a cascade multi pack -> (per_image[i][o][c] = (dets, ids), [ROI count per image]): the multi pack with
    num_outputs * num_classes slots per image, output-major."""
    flat, rois = unpack_detections_multi(pack_host, num_images, num_outputs * num_classes, cap, out_cap)
    return [[row[o * num_classes:(o + 1) * num_classes] for o in range(num_outputs)] for row in flat], rois
