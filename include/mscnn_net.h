/*
 * mscnn_net.h -- C ABI of libmscnn_caffe.so: the Caffe-compatible host runtime (caffe::Net<float> and the
 * caffe::Layer<float> subclasses in mscnn_amd/host) for foreign-language callers.  This is what a MATLAB MEX /
 * Python wrapper binds instead of the reference's matcaffe (matlab/+caffe/private/caffe_.cpp:253 get_net,
 * :300-306 net_forward, :57-107 blob get/set) or pycaffe (python/caffe/_caffe.cpp).
 * C++ callers use the caffe:: classes directly (mscnn_amd/host/include/caffe/caffe.hpp).
 *
 * All functions return 0 on success; on failure the text is available from mscnn_net_last_error().
 * A net and everything it owns lives on ONE device and must be used from ONE host thread (the reference's
 * Caffe singleton is thread-local, src/caffe/common.cpp:12-20).
 */
#ifndef MSCNN_NET_H_
#define MSCNN_NET_H_

#include <stddef.h>

#if defined(__GNUC__)
#define MSCNN_NET_API __attribute__((visibility("default")))
#else
#define MSCNN_NET_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mscnn_net mscnn_net;

MSCNN_NET_API const char* mscnn_net_last_error(void);

/* caffe.Net(prototxt, 'test') -- Net::Net(file, TEST), src/caffe/net.cpp:31-46.  device: HIP device ordinal;
 * device < 0 builds the graph without touching a device (shape / naming inspection only; forward then fails). */
MSCNN_NET_API int mscnn_net_create_from_file(const char* prototxt_path, int device, mscnn_net** out);
MSCNN_NET_API int mscnn_net_create_from_string(const char* prototxt_text, int device, mscnn_net** out);
/* flags: MSCNN_NET_NO_FUSION builds the net without the Net-level operator fusion (every layer runs its own kernel, as in the
 * reference; results are bit-identical, roi_pool_org / roi_pool_ctx style intermediate blobs are written eagerly). */
#define MSCNN_NET_NO_FUSION 1
MSCNN_NET_API int mscnn_net_create_from_string_ex(const char* prototxt_text, int device, unsigned flags, mscnn_net** out);
MSCNN_NET_API void mscnn_net_destroy(mscnn_net* net);
/* net.copy_from(weights) -- Net::CopyTrainedLayersFrom, net.cpp:750-803: a binary NetParameter (.caffemodel), or -- for a path
 * ending in ".h5", like the reference (net.cpp:788-795) -- an HDF5 snapshot (Net::CopyTrainedLayersFromHDF5, net.cpp:806-848). */
MSCNN_NET_API int mscnn_net_load_caffemodel(mscnn_net* net, const char* path);
/* HIP stream (hipStream_t as void*) for every subsequent call on this thread; NULL = default stream.
 * The setting is per host THREAD, not per net (it lives in the thread's Caffe singleton, as the reference's cuBLAS handle does).
 * "The net's stream" below always means: the stream that is set on the calling thread at the time of the call.  A net's frame --
 * set_blob / set_image*, forward, the detect and proposals calls, the pinned slots and events of detect_begin / detect_end, the
 * numerics watch, the tracker, render, crops -- is enqueued on that stream, under the STREAM CONTRACT of mscnn_hip.h; calls that return host
 * data wait for that stream only, not for the device (a buffer that has to grow is the exception: hipFree waits for the device).  One thread may drive several nets on several streams by setting the stream
 * in front of each net's calls (tests/test_gpu_net_streams.py).  A net must not be switched to another stream while work of its own
 * is still in flight on the old one unless the caller orders the two streams (an event, or a synchronisation): its blobs, packs and
 * tables are shared between its frames.  The caller keeps the stream alive while it is set.  mscnn_amd.net: set_stream, on_stream. */
MSCNN_NET_API int mscnn_net_set_stream(void* stream);

/* graph introspection (Net::layer_names / blob_names / layers()[i]->blobs()) */
MSCNN_NET_API int mscnn_net_num_layers(const mscnn_net* net);
MSCNN_NET_API const char* mscnn_net_layer_name(const mscnn_net* net, int layer);
MSCNN_NET_API const char* mscnn_net_layer_type(const mscnn_net* net, int layer);
MSCNN_NET_API int mscnn_net_layer_index(const mscnn_net* net, const char* name);           /* -1 if absent */
MSCNN_NET_API int mscnn_net_layer_num_bottoms(const mscnn_net* net, int layer);
MSCNN_NET_API int mscnn_net_layer_num_tops(const mscnn_net* net, int layer);
MSCNN_NET_API const char* mscnn_net_layer_bottom(const mscnn_net* net, int layer, int i);  /* blob name */
MSCNN_NET_API const char* mscnn_net_layer_top(const mscnn_net* net, int layer, int i);
MSCNN_NET_API int mscnn_net_layer_num_params(const mscnn_net* net, int layer);
MSCNN_NET_API int mscnn_net_layer_param_shape(const mscnn_net* net, int layer, int param, int* dims8, int* ndim);
/* The layer's LayerParameter in prototxt text form (valid until the next call on this thread). */
MSCNN_NET_API const char* mscnn_net_layer_param_text(const mscnn_net* net, int layer);
MSCNN_NET_API int mscnn_net_layer_fused_away(const mscnn_net* net, int layer);              /* 1: ReLU folded into its producer */
MSCNN_NET_API const char* mscnn_net_layer_kernel(const mscnn_net* net, int layer);          /* conv / InnerProduct kernel family; "roialign_ave_pair" for the first ROIAlign layer of a head the last forward ran in one pass; "" otherwise */
MSCNN_NET_API double mscnn_net_layer_flops(const mscnn_net* net, int layer);                /* of the last forward */
/* Roofline accounting of Convolution layers: FLOPs the MFMA pipe executes (Winograd forms: fewer than the algorithmic
 * count above) and, with conv profiling on, the HIP-event time of the last forward split into {input transform, MFMA GEMM
 * kernels, output transform} (direct kernels: {0, total, 0}); non-convolution layers report zeros. */
MSCNN_NET_API double mscnn_net_layer_executed_flops(const mscnn_net* net, int layer);
MSCNN_NET_API int mscnn_net_set_conv_profiling(mscnn_net* net, int on);
MSCNN_NET_API int mscnn_net_layer_stage_ms(const mscnn_net* net, int layer, float ms_out[3]);
/* Convolution algorithm of one layer (layer < 0: all): mscnn_conv_algo of include/mscnn_hip.h (0 auto, 1 direct,
 * 2 / 3 Winograd F(2x2,3x3) / F(3x3,3x3) wherever legal); tuning knobs = mscnn_conv_desc::tune_* (A/B runs). */
MSCNN_NET_API int mscnn_net_set_conv_algo(mscnn_net* net, int layer, int algo);
MSCNN_NET_API int mscnn_net_set_conv_tuning(mscnn_net* net, int layer, int variant, int grid, int flags);
/* fp32 kernel of one InnerProduct layer (layer < 0: all): 0 = auto (fc6-class shapes on the plane-GEMM kernel, mscnn_inner_product_wg_*),
 * 1 = always the stream-K kernel of gemm.hip (A/B runs, second witness).  mscnn_net_layer_kernel reports what the last forward ran. */
MSCNN_NET_API int mscnn_net_set_inner_product_algo(mscnn_net* net, int layer, int algo);
/* Arithmetic of the MFMA layers of the whole net: "f32" (default: the path that matches the reference within 1e-4) or "f16"
 * (fp16 operands, fp32 accumulate, no reference counterpart -- BASELINE config 5): 3x3 stride-1 convolutions and InnerProduct
 * layers with N >= 64 switch, everything else keeps its fp32 kernel.  "f16x3": the convolutions that run Winograd F(3x3,3x3)
 * multiply their planes on the fp16 MFMA pipe with every fp32 operand split exactly into fp16 hi + lo (three products, fp32
 * accumulate; MSCNN_CONV_ALGO_WINO_F3_X3) -- fp32-grade results held to the SAME parity gates as "f32", max |x| handed from
 * layer to layer on the device.  mscnn_net_layer_dtype: what layer i really runs. */
MSCNN_NET_API int mscnn_net_set_precision(mscnn_net* net, const char* dtype);
MSCNN_NET_API const char* mscnn_net_layer_dtype(const mscnn_net* net, int layer);
/* Numerics are SAFE BY DEFAULT (no call needed; the reference's flow -- Net(prototxt, TEST); CopyTrainedLayersFrom; Forward,
 * net.cpp:750-785, 544-555 -- stays as it is): the Winograd forms AUTO picks carry ~10x the rounding error of the direct sum, so
 * every Convolution layer compares its Winograd result with the direct k-ordered kernel on the FIRST bottom it sees after
 * construction or a weight change (mscnn_net_set_param, mscnn_net_copy_trained_from, Layer::OnWeightsChanged), metric
 * max |dy| / max(1, |y|, rms(y)), tolerance 5e-5, and when it is off switches to the direct kernel and recomputes its tops before
 * that forward returns.  Cost: the first forward after a weight change runs each Winograd layer twice.
 *   mscnn_net_set_auto_calibrate(net, tol): tol = 0 is the opt-OUT; tol > 0 re-arms every layer's check with that tolerance.
 *   mscnn_net_auto_calibrate_state: *checks = first-forward checks done so far; returns how many layers fell back and writes up to
 *   cap of their indices; mscnn_net_layer_calibration_err gives each layer's last measured value.
 * mscnn_net_calibrate_numerics is the same check on demand (call after a forward on representative input): every convolution that
 * runs a Winograd form is re-computed with the direct kernel on the same bottom; layers over tol run the direct kernel from then on.
 * *num_switched = how many. */
MSCNN_NET_API int mscnn_net_set_auto_calibrate(mscnn_net* net, double tol);
/* Chains of same-resolution F(4x4,3x3) convolutions (conv2_1 -> conv2_2, conv3_1 -> 3_2 -> 3_3, conv4_1 -> 4_2 -> 4_3; mscnn_hip.h:
 * mscnn_conv2d_fwd_chain_f32): inside a forward the blob between two members is not written -- the producer's output stage writes the
 * consumer's transform planes.  mscnn_net_get_blob / _blob_device on such a blob re-run its producer on demand (bit-identical to the
 * unchained forward; the reference's contract that every blob holds its layer's output after Forward, net.cpp:544-555, is kept for
 * every reader that goes through this ABI).  ON by default (with the other Net-level fusions); on = 0 writes every blob in every
 * forward (MSCNN_NO_CHAIN=1 does the same process-wide). */
MSCNN_NET_API int mscnn_net_set_chain_fusion(mscnn_net* net, int on);
/* BoxOutput of a batched net (more than one image in its bottoms) runs every image side by side (mscnn_hip.h:
 * mscnn_boxoutput_batch_fwd_f32): OFF by default (image after image, mscnn_boxoutput_fwd_f32) until the batched op has been timed; on = 1 selects it.  The tops are
 * bit-identical either way, and a net of one image always takes mscnn_boxoutput_fwd_f32. */
MSCNN_NET_API int mscnn_net_set_boxoutput_one_pass(mscnn_net* net, int on);
/* The ROIAlign head of the WiderFace cascade -- roi_grid_org / roi_pool_org / roi_grid_ctx / roi_pool_ctx / roi_pool, once per stage --
 * in one launch (mscnn_hip.h: mscnn_roialign_ave_pair_fwd_f32).  A head is registered at construction: two ROIAlign layers that read
 * the same feature blob and the same ROI blob (through Split layers) with equal pooled_h / pooled_w / spatial_scale, each top read by
 * exactly one Pooling layer that is AVE, kernel 2, stride 1, pad 0, those two tops read only by one Concat on axis 1.  OFF by default
 * until the one-pass form has been timed against the chain on the frames that matter: a net that never calls this runs the launches it
 * always ran.  on = 1: in a forward whose range holds all five layers the first ROIAlign layer writes the Concat's top and the other
 * four launch nothing; a range that holds part of a head runs its layers stand-alone.  The tops are bit-identical either way, and so
 * is every blob read through this ABI: mscnn_net_get_blob / _blob_device on a grid or pooled blob the forward did not write run the
 * skipped layers on the same bottoms first, and so do a weight change, a reshape and a partial forward that does not run the head.
 *   mscnn_net_roialign_pairs: how many heads the net registered; writes up to cap indices of their first ROIAlign layers. */
MSCNN_NET_API int mscnn_net_set_roialign_one_pass(mscnn_net* net, int on);
MSCNN_NET_API int mscnn_net_roialign_pairs(const mscnn_net* net, int* first_layers, int cap);
/* The pairs the net registered at construction: producers[i] -> consumers[i] (layer indices; consumers[i] = -1: a top that only its
 * fused 2x2 pooling reads).  Returns their number and writes up to cap of them; whether a pair actually runs chained is decided per
 * forward (both planned kernels on the fp32 F(4x4,3x3) path, no numerical check pending, both layers inside the range). */
MSCNN_NET_API int mscnn_net_chain_pairs(const mscnn_net* net, int* producers, int* consumers, int cap);
MSCNN_NET_API int mscnn_net_auto_calibrate_state(const mscnn_net* net, int* checks, int* switched_layers, int cap);
MSCNN_NET_API int mscnn_net_calibrate_numerics(mscnn_net* net, double tol, int* num_switched);
MSCNN_NET_API double mscnn_net_layer_calibration_err(const mscnn_net* net, int layer);
/* The same comparison on live frames (the numerics watch): every period-th whole forward looks at ONE Winograd layer (round robin) --
 * its bottom and top blobs are written in that frame (it stays in its convolution chain), and one band of it (a few rows / images: ~30 us of direct-kernel work; round robin too) is
 * recomputed with the direct kernel BEHIND the frame on the same stream, with no host synchronisation; the verdict is collected by a
 * later forward, and a layer off by more than tol runs the direct kernel from the frame after.  No frame waits for a check: a watch
 * frame is 2 - 8 % longer (7s-576), the others not at all.  ON by default with period 25, tol 5e-5 (~0.1 % of a stream); period 0
 * switches the watch off.  _state: waits for a verdict that is still out, then *checks = band checks done so far; returns how many
 * layers were switched and writes up to cap of their indices. */
MSCNN_NET_API int mscnn_net_set_numerics_watch(mscnn_net* net, int period, double tol);
MSCNN_NET_API int mscnn_net_numerics_watch_state(const mscnn_net* net, int* checks, int* switched_layers, int cap);
MSCNN_NET_API int mscnn_net_num_blobs(const mscnn_net* net);
MSCNN_NET_API const char* mscnn_net_blob_name(const mscnn_net* net, int blob);
MSCNN_NET_API int mscnn_net_blob_shape(const mscnn_net* net, const char* name, int* dims8, int* ndim);
MSCNN_NET_API int mscnn_net_num_inputs(const mscnn_net* net);
MSCNN_NET_API int mscnn_net_num_outputs(const mscnn_net* net);
MSCNN_NET_API const char* mscnn_net_output_name(const mscnn_net* net, int i);               /* alphabetical, net.cpp:267-274 */

/* weights: layer->blobs()[param]  (host fp32, Caffe layout).  The setter marks the layer's packed copy stale. */
MSCNN_NET_API int mscnn_net_set_param(mscnn_net* net, int layer, int param, const float* host, size_t count);
MSCNN_NET_API int mscnn_net_get_param(mscnn_net* net, int layer, int param, float* host, size_t count);

/* blob.set_data / get_data.  *_device copy device->device on the net's stream (no PCIe). */
MSCNN_NET_API int mscnn_net_set_blob(mscnn_net* net, const char* name, const float* host, size_t count);
MSCNN_NET_API int mscnn_net_set_blob_device(mscnn_net* net, const char* name, const float* dev, size_t count);
/* The MATLAB pre-processing in front of net.forward (run_mscnn_detection.m:64-69), on the device: a decoded uint8 RGB frame
 * [org_h][org_w][3] (host memory, or device memory when on_device != 0) is resized to the input blob's H x W (imresize
 * semantics), swapped to BGR, mean-subtracted (mean_bgr == NULL: {104,117,123}) and written into blob `name`. */
MSCNN_NET_API int mscnn_net_set_image(mscnn_net* net, const char* name, const unsigned char* img_rgb, int on_device,
                                      int org_h, int org_w, const float* mean_bgr);
/* The batched set_image: `count` frames, frame b uint8 [org_h[b]][org_w[b]][3] (imgs_rgb: a host array of host pointers, or of
 * device pointers when on_device != 0), each resized to the blob's H x W and written into slice b of blob `name`.  Requires
 * count == num() and channels() == 3; refused before anything is written. */
MSCNN_NET_API int mscnn_net_set_images(mscnn_net* net, const char* name, const unsigned char* const* imgs_rgb, int on_device,
                                       const int* org_h, const int* org_w, int count, const float* mean_bgr);
/* VIEWS of one or more frames as the images of the blob: a frame and its mirror, the tiles of a frame too large for one forward
 * (mscnn_hip.h: mscnn_preprocess_views_u8_f32; the struct is repeated here so that this header stands alone).  frames_rgb: a host
 * array of num_frames host pointers (device pointers when on_device != 0), frame f uint8 [org_h[f]][org_w[f]][3]; view v = the window
 * [y0, y0 + h) x [x0, x0 + w) of frame views[v].frame, reversed along x when flip_x, resized to the blob's H x W and written into
 * slice v -- bit for bit what mscnn_net_set_image writes for a contiguous host copy of that window (mirrored with [:, ::-1]).  A host
 * frame is uploaded ONCE, whatever the number of its views.  Requires count == num() and channels() == 3.  Refused before anything
 * is uploaded or written, naming the value: a null pointer, num_frames < 1, a frame of size <= 0, a view's frame outside
 * [0, num_frames), a window that is empty or not inside its frame, a flip_x that is neither 0 nor 1, a net built with device < 0.
 * No pin on the reference: its scripts pre-process whole frames only. */
#ifndef MSCNN_PREPROCESS_VIEW_DEFINED
#define MSCNN_PREPROCESS_VIEW_DEFINED
typedef struct { int frame; int x0, y0, w, h; int flip_x; } mscnn_preprocess_view;
#endif
MSCNN_NET_API int mscnn_net_set_image_views(mscnn_net* net, const char* name, const unsigned char* const* frames_rgb, int on_device,
                                            const int* org_h, const int* org_w, int num_frames, const mscnn_preprocess_view* views,
                                            int count, const float* mean_bgr);
MSCNN_NET_API int mscnn_net_get_blob(mscnn_net* net, const char* name, float* host, size_t capacity, size_t* count);
MSCNN_NET_API const float* mscnn_net_blob_device_ptr(mscnn_net* net, const char* name);

/* net.forward_prefilled(): Net::ForwardFromTo(0, L-1), net.cpp:544-575.  from/to: layer range, (0, -1) = all. */
MSCNN_NET_API int mscnn_net_forward(mscnn_net* net);
MSCNN_NET_API int mscnn_net_forward_from_to(mscnn_net* net, int from, int to);
MSCNN_NET_API int mscnn_net_reshape(mscnn_net* net);
/* Input reshape: blob->Reshape(dims) on a net input followed by Net::Reshape() (net.cpp:743-747; matcaffe's
 * net.blobs('data').reshape([w h c n]); net.reshape()) -- another batch size (dims[0]) or frame size without re-creating the net.
 * dims in Caffe's order (N, C, H, W).  The whole path is batch-generic like the reference's (conv_layer.cpp:25-40 loops over num_,
 * box_output_layer.cpp:107 over images, roi_pooling_layer.cpp:62-66 takes the image from column 0 of every ROI): a forward of
 * N images returns the ROI blobs grouped by image; the final stage then runs once per image (mscnn_net_detect_image). */
MSCNN_NET_API int mscnn_net_reshape_input(mscnn_net* net, const char* name, const int* dims, int ndim);
/* Health of the plane-GEMM kernel's stream-K hand-off (mscnn_hip.h: mscnn_wgemm_handoff_event).  A hand-off that times out (a
 * workgroup of the persistent grid was not co-resident: CU masking, a partition mode, another stream's kernels) can never hand out a
 * wrong frame through this ABI: the Net reads the kernel's status word wherever it synchronises anyway -- behind BoxOutput's
 * row-count read inside a forward, behind the copy of mscnn_net_detect and of mscnn_net_get_blob -- and on an event forces
 * whole-tile scheduling for the rest of the process and runs the frame again before the call returns (cost: one frame twice, once).
 * Returns how many events this net has answered so far; *whole_tiles_forced (may be NULL) = 1 once the process runs on whole tiles.
 * (mscnn_net_detect_device + the RCCL exchange, and C++ callers that read Blob::cpu_data() themselves, synchronise outside the Net:
 * they call caffe::Net::HandoffRecover() / look at mscnn_wgemm_handoff_event() behind their own synchronisation.) */
MSCNN_NET_API int mscnn_net_handoff_state(const mscnn_net* net, int* whole_tiles_forced);
/* `caffe time`-style per-layer HIP-event timing (tools/caffe.cpp:380-400); serialises the layers. */
MSCNN_NET_API int mscnn_net_set_layer_timing(mscnn_net* net, int on);
MSCNN_NET_API float mscnn_net_layer_ms(const mscnn_net* net, int layer);

/*
 * Final detection stage on the net's own output blobs (bbox_pred, cls_pred, proposals_score), on the device:
 * the MATLAB post-processing of run_mscnn_detection.m:75-120 + bbNms.m:112-126.  Only the detections
 * (dets_host[cap][5] doubles [x y w h prob], ids_host[cap] ROI row per detection) cross PCIe.
 */
typedef struct {
  int cls_id;                       /* 1-based class column (car = 2 for the KITTI car nets) */
  float bbox_mean[4], bbox_std[4];  /* [0 0 0 0], [.1 .1 .2 .2] in the scripts */
  float proposal_thr;               /* -10 */
  double ratio_h, ratio_w;          /* net input size / original image size */
  double org_h, org_w;              /* original image size (clip bounds) */
  double nms_overlap;               /* 0.5 */
} mscnn_detect_params;
/* bbNms's user knobs for EVERY detect call on this net from now on -- `pNms.type / pNms.ovrDnm` (and bbNms's thr) at the top of the
 * reference scripts; pNms.overlap stays in mscnn_detect_params.  The struct, its field encodings and what is refused ('ms', 'cover',
 * 'none', out-of-range values: an error naming the value, the setting unchanged) are those of include/mscnn_hip.h, repeated here
 * so that this header stands alone.  NULL = the defaults (nmsMax greedy, union, thr -inf, no det_thr), under which every call runs
 * exactly the kernels it ran before this setting existed.  det_thr is the plain stage's (widerface/run_mscnn_detection.m:139-143);
 * the cascade calls take theirs as an argument and fail, naming the value, while the setting's det_thr is not 0.  A forward with more than 4032 ROI rows per image runs the tiled
 * per-segment path, which has the default setting only: a detect call fails there, naming the limit, instead of ignoring the
 * setting.  The new modes have not been timed on the full nets. */
#ifndef MSCNN_NMS_PARAMS_DEFINED
#define MSCNN_NMS_PARAMS_DEFINED
typedef struct {
  int type;          /* 0 = 'maxg', 1 = 'max' */
  int ovr_dnm;       /* 0 = 'union', 1 = 'min' */
  double thr;        /* -HUGE_VAL = bbNms's default -inf; rows with !(prob > thr) are dropped */
  float det_thr;     /* 0 = off; > 0: rows with !(prob >= det_thr) are dropped (plain stage only) */
} mscnn_nms_params;
#endif
MSCNN_NET_API int mscnn_net_set_nms(mscnn_net* net, const mscnn_nms_params* nms);
MSCNN_NET_API int mscnn_net_get_nms(const mscnn_net* net, mscnn_nms_params* out);
MSCNN_NET_API int mscnn_net_detect(mscnn_net* net, const mscnn_detect_params* p, double* dets_host, int* ids_host,
                                   int cap, int* num_dets, int* num_rois);
/* The same stage for a STREAM of frames (batch-1 nets), pipelined: _begin runs the final stage of the forward just done into the
 * device pack, enqueues ONE copy of it into one of two pinned host slots behind an event on the net's stream, and returns at once --
 * the caller goes on with the next frame (set_blob / forward); _end waits for the OLDEST frame in flight and unpacks it: frame i's
 * detections reach the host under frame i + 1's trunk instead of idling the device for a host round trip per frame.  At most two
 * frames in flight; cap as in mscnn_net_detect_device (BoxOutput's max_nms_num bounds R).  Results are bit-identical to
 * mscnn_net_detect.  A stream-K hand-off time-out while frames are in flight can not be answered by a re-run here (the input blob
 * already holds a later frame): _end then FAILS, naming it, after forcing whole-tile scheduling -- submit the frames begun since the
 * last _end again. */
MSCNN_NET_API int mscnn_net_detect_begin(mscnn_net* net, const mscnn_detect_params* p, int cap);
MSCNN_NET_API int mscnn_net_detect_end(mscnn_net* net, double* dets_host, int* ids_host, int cap, int* num_dets, int* num_rois);
/* The same stage for image `image` of a batched forward (the MATLAB stage is per image: its NMS never mixes images; mscnn_net_detect
 * itself refuses a net whose input holds more than one image).  ids_host = rows of the net's ROI blobs (bbox_pred, cls_pred,
 * proposals_score), *num_rois = the image's own ROI count. */
MSCNN_NET_API int mscnn_net_detect_image(mscnn_net* net, const mscnn_detect_params* p, int image, double* dets_host, int* ids_host,
                                         int cap, int* num_dets, int* num_rois);
/* The final stage of EVERY image and class of the last forward in one pass: one stream synchronisation per call instead of one per
 * (image, class), three launches (mscnn_hip.h: mscnn_detections_multi_fwd) instead of three per pair.  p[num_images * num_classes],
 * indexed [image * num_classes + class]: each image may carry its own ratios and original size.  num_images must equal the input's
 * N (1 is legal and equals mscnn_net_detect).  Output segment after segment, image-major: seg_dets[s] detections of segment s in
 * dets_host / ids_host (ids = rows of the net's ROI blobs, as mscnn_net_detect_image), image_rois[num_images] (may be NULL) = each
 * image's ROI count.  More detections than cap is an error naming the numbers, never a truncation.  Every segment is bit-identical to
 * mscnn_net_detect_image of its image and class.  A per-image row bound over 4032 (BoxOutput max_nms_num 0) runs the per-segment
 * path into the same layout. */
MSCNN_NET_API int mscnn_net_detect_multi(mscnn_net* net, const mscnn_detect_params* p, int num_images, int num_classes, double* dets_host,
                                         int* ids_host, int cap, int* seg_dets, int* image_rois);
/* The same into a device pack of mscnn_net_detect_multi_pack_bytes(num_images, num_classes, cap) bytes in HBM (layout: mscnn_hip.h,
 * mscnn_detections_multi_fwd; cap >= num_classes x the forward's ROI count, else an error); asynchronous on the net's stream, *pack_dev
 * valid until the next detect call on this net.  mscnn_net_unpack_detections_multi reads one host copy of it (out_cap = rows of
 * dets_host / ids_host; refuses a pack of another shape or capacity and a corrupt one). */
MSCNN_NET_API size_t mscnn_net_detect_multi_pack_bytes(int num_images, int num_classes, int cap);
MSCNN_NET_API int mscnn_net_detect_multi_device(mscnn_net* net, const mscnn_detect_params* p, int num_images, int num_classes, int cap,
                                                const void** pack_dev);
MSCNN_NET_API int mscnn_net_unpack_detections_multi(const void* pack_host, int num_images, int num_classes, int cap, double* dets_host,
                                                    int* ids_host, int out_cap, int* seg_dets, int* image_rois);

/* The proposal half of the scripts' result (run_mscnn_detection.m:75-91: `final_proposals{k}`, what the drivers would write to
 * proposals/<comp_id>.txt and what their `show` path indexes with the detections' ids) for EVERY image of the last forward in one
 * pass (mscnn_hip.h: mscnn_proposals_multi_fwd), from the net's proposals_score blob on the device.  p[num_images]: of each image's
 * params only proposal_thr, ratio_h and ratio_w are read.  num_images must equal the input's N.  Output image after image:
 * props_host[cap][5] doubles [x y w h score] (fp32 extents, filtered as the final stage filters, then divided by the ratios in
 * double), rows_host[cap] = the row of the net's ROI blobs each came from -- the convention of mscnn_net_detect_multi's ids, so the
 * script's proposals(bbs_show(:,6),:) is a join on that column --, image_props[num_images] = rows of each image, image_rois[num_images]
 * (may be NULL) = its ROI count.  Blocking: the kernel writes the pack into host-coherent pinned memory and the call synchronises
 * once.  More rows than cap is an error naming the numbers.  A net without a proposals_score blob is refused, naming the blob, and
 * so is a cascade deploy (a net with a DecodeBBox layer, named in the error): its BoxOutput has the blob, but the cascade drivers
 * output no proposals.  No pin on the reference (no MATLAB): the check is a numpy restatement. */
MSCNN_NET_API int mscnn_net_proposals_multi(mscnn_net* net, const mscnn_detect_params* p, int num_images, double* props_host,
                                            int* rows_host, int cap, int* image_props, int* image_rois);
/* The same into a device pack of mscnn_net_detect_multi_pack_bytes(num_images, 1, cap) bytes (cap >= the forward's ROI count, else an
 * error); asynchronous on the net's stream, *pack_dev valid until the next detect / proposals call on this net.
 * mscnn_net_unpack_detections_multi(pack, num_images, 1, cap, ...) reads one host copy of it. */
MSCNN_NET_API int mscnn_net_proposals_multi_device(mscnn_net* net, const mscnn_detect_params* p, int num_images, int cap,
                                                   const void** pack_dev);
/* The RPN-only run: Net::ForwardFromTo(0, L), L = the BoxOutput layer whose second top is proposals_score (written to *last_layer,
 * may be NULL) -- MS-CNN as a proposal generator, without the detection sub-network.  The ROI pooling's maps are not enqueued under
 * BoxOutput (nothing of this call reads them), the call is not a whole forward for the numerics watch, and a later mscnn_net_forward
 * is bit-identical to one on a fresh net.  mscnn_net_proposals_multi then reads the blob as after a whole forward; the detect calls
 * would read the sub-net's blobs of an EARLIER forward. */
MSCNN_NET_API int mscnn_net_forward_proposals(mscnn_net* net, int* last_layer);
/* The opposite half: the detection sub-network on caller-supplied ROIs -- a tracker's predictions, another detector's proposals,
 * ground-truth boxes, a proposals file --, without conv5_x / conv6_1 / the LFCN heads / pool6 / BoxOutput.  rows: R rows in host memory,
 * or in device memory when on_device != 0, in one of the two forms of mscnn_rois_ingest_f32 (include/mscnn_hip.h), repeated here
 * so that this header stands alone:
 *   coords 0 (MSCNN_ROIS_NET)    fp32 [image x1 y1 x2 y2 score] in net-input coordinates, the layout of proposals_score; copied bit
 *                                for bit; p may be NULL
 *   coords 1 (MSCNN_ROIS_IMAGE)  double [image x y w h score] in original-image pixels, 0-based image index, the rows of
 *                                mscnn_net_proposals_multi; p[num_images]: of each image's params only ratio_h and ratio_w are read;
 *                                x1 = (float)(x * ratio_w), x2 = (float)((x + w) * ratio_w), y likewise with ratio_h
 * Rows must be finite, carry a whole image index in [0, num_images) and be grouped by image in ascending order (an image may have
 * none): they are checked on the device, and a bad row fails the call naming the row and the reason; the sub-net is then not run, the
 * ROI blobs hold the one all-zero row BoxOutput emits when nothing survives, and the sub-net's blobs are those of an earlier forward.
 * L = the BoxOutput layer mscnn_net_forward_proposals looks up (or a BoxOutput layer with one top that feeds the ROI layers), K = the
 * last layer in front of L that a layer behind L depends on other than through L's tops (relu4_3 and its Split in the KITTI / Caltech
 * deploys; the "-2x" nets' Deconvolution sits behind L).  The call writes the rows into L's tops as L itself would have (one launch,
 * R is known before anything is enqueued: no host round trip inside the frame), runs layers 0 .. K when run_trunk != 0, then layers
 * L + 1 .. last.  With run_trunk = 0 the feature blobs of the previous forward are used as they are: the caller vouches that they belong
 * to the frame these ROIs are meant for.  image_rois [num_images] (may be NULL) = rows of each image.
 * Refused before anything is enqueued, naming the value: R above the row bound of L (its max_nms_num x images: detection packs and
 * workspaces are sized by it) or below 1, num_images other than the input's N, a net without ROI layers, a net built with device < 0.
 * Afterwards every blob from L's tops to the net's outputs holds, bit for bit, what mscnn_net_forward writes when BoxOutput itself
 * selects these rows -- blobs a fusion leaves unwritten and mscnn_net_get_blob materialises on demand included --, and the detect,
 * detect_multi, detect_cascade_multi and proposals_multi calls work on the result unchanged.  (Under set_precision "f16x3" the
 * sub-net measures max |x| of its input itself, as in any partial forward: the same gates, not the same bits.)  The layers between K
 * and L are not run: their blobs, and with run_trunk = 0 the trunk's, are those of an EARLIER forward.  The ROI pooling's maps are not
 * enqueued ahead (roi_c1 builds them itself), the call is not a whole forward for the numerics watch, and a later mscnn_net_forward is
 * bit-identical to one on a fresh net.  A stream-K hand-off time-out noticed behind such a frame (mscnn_net_handoff_state) runs the
 * same two ranges again around the rows, which are still in L's tops -- never a range that holds L.  Measured once (profiles/forward_rois.txt): slower than mscnn_net_forward today. */
MSCNN_NET_API int mscnn_net_forward_rois(mscnn_net* net, const void* rows, int on_device, int coords, int R,
                                         const mscnn_detect_params* p /* num_images of them; NULL for net-input coordinates */,
                                         int num_images, int run_trunk, int* image_rois /* may be NULL */);
/* L and K of mscnn_net_forward_rois for this net (layer indices; K = -1: nothing in front of L is needed).  Fails, as the call itself
 * does, for a net without ROI layers.  Works on a net built with device < 0. */
MSCNN_NET_API int mscnn_net_forward_rois_layers(const mscnn_net* net, int* L, int* K);


/* Final stage of the cascade drivers (examples/kitti_car/run_cascademscnn.m:84-127) for ONE cascade output nn: the decoded boxes
 * of stage nn (`bbox_blob`, e.g. "output_bbox_3rd"), its in-net probabilities (`prob_blob`, "cls_prob_3rd" / "cls_prob_3rd_avg")
 * and the proposals it refined (`proposal_blob`, "proposals_3rd"), all read from the net on the device: rescale, clip, drop
 * zero-size proposals, optional det_thr (> 0), bbNms.  Same outputs as mscnn_net_detect; p->bbox_mean/std, proposal_thr unused. */
MSCNN_NET_API int mscnn_net_detect_cascade(mscnn_net* net, const mscnn_detect_params* p, float det_thr, const char* bbox_blob,
                                           const char* prob_blob, const char* proposal_blob, double* dets_host, int* ids_host,
                                           int cap, int* num_dets, int* num_rois);
/* The cascade stage for EVERY image, cascade output and class of the last forward in one pass (the loops of
 * run_cascademscnn.m:91-143 over a whole batch): three launches per 32 segments (mscnn_hip.h: mscnn_detections_cascade_multi_fwd)
 * and one stream synchronisation, and -- unlike mscnn_net_detect_cascade, which treats the blobs as one list -- never an NMS across
 * images.  bbox_blobs / prob_blobs / proposal_blobs[num_outputs], 1 <= num_outputs <= 4: the blob triple of each cascade output
 * (equal row counts throughout).  p[num_images * num_outputs * num_classes], indexed [(image * num_outputs + output) * num_classes
 * + class]: cls_id, ratios, original size, nms_overlap (bbox_mean / bbox_std / proposal_thr unused); det_thr: one value per call.
 * num_images must equal the input's N.  Output segment after segment in that order, as mscnn_net_detect_multi with num_outputs *
 * num_classes in the role of num_classes: seg_dets[s], ids = rows of the net's blobs, image_rois[num_images] (may be NULL).  Every
 * segment is bit-identical to mscnn_detections_cascade_fwd on the image's rows of that output's blobs; at N = 1, one output and one
 * class it equals mscnn_net_detect_cascade.  A per-image row bound over 4032 runs the per-segment path into the same layout. */
MSCNN_NET_API int mscnn_net_detect_cascade_multi(mscnn_net* net, const mscnn_detect_params* p, int num_images, int num_outputs,
                                                 int num_classes, const char* const* bbox_blobs, const char* const* prob_blobs,
                                                 const char* const* proposal_blobs, float det_thr, double* dets_host, int* ids_host,
                                                 int cap, int* seg_dets, int* image_rois);
/* The same into a device pack of mscnn_net_detect_cascade_multi_pack_bytes(...) bytes in HBM (cap >= num_outputs x num_classes x the
 * forward's ROI count, else an error); asynchronous on the net's stream, *pack_dev valid until the next detect call on this net.
 * mscnn_net_unpack_detections_multi(pack, num_images, num_outputs * num_classes, cap, ...) reads one host copy of it. */
MSCNN_NET_API size_t mscnn_net_detect_cascade_multi_pack_bytes(int num_images, int num_outputs, int num_classes, int cap);
MSCNN_NET_API int mscnn_net_detect_cascade_multi_device(mscnn_net* net, const mscnn_detect_params* p, int num_images, int num_outputs,
                                                        int num_classes, const char* const* bbox_blobs, const char* const* prob_blobs,
                                                        const char* const* proposal_blobs, float det_thr, int cap,
                                                        const void** pack_dev);

/* Several forwards of a frame, ONE NMS: input sizes (multi-scale testing), a mirrored frame, tiles of a frame too large for one
 * forward (mscnn_hip.h: mscnn_detections_candidates_*, mscnn_detections_merge_fwd).  Between _begin and _end the caller may
 * reshape_input, set_image(s), forward, forward_rois -- everything that leaves the three blobs behind -- and calls one _add after each
 * forward: the rows that survive the final stage's row transform (its filters and the net's sticky set_nms thr / det_thr included)
 * stay on the device, per segment, in original-image coordinates.  _end runs the sort and the NMS once over each segment's list.
 *   _begin   reserves and resets the lists: num_images x num_classes segments of cand_cap candidate slots each.  For the cascade
 *            form num_classes stands for num_outputs x num_classes.
 *   _add     p[num_images * num_classes] as in mscnn_net_detect_multi, describing THIS forward's view of each image: ratios = the
 *            net's input size / the view's size, org_h / org_w = the view's size (the tile, or the whole frame).  view[num_images]
 *            (NULL: the identity) places the view in the original image, in double, on the box [x y w h] the row transform returned:
 *                x' = flip_x ? (double)(float)org_w - (x + w) : x;   x' += off_x;   y' = y + off_y;   w, h, prob untouched
 *            (a frame mirrored with [:, ::-1] has flip_x = 1; a tile has its corner as the offset).  The cascade rows keep their
 *            w = x2 - x1 + 1 convention under the same formula.  The pass index is the number of adds since _begin (at most 128).
 *            Refused before anything is enqueued, naming the values: the sum over the adds so far of each forward's ROI row count
 *            could pass cand_cap (the host knows every R_all: never a truncation); an nms_overlap other than the one the segment
 *            had at the first add (both values named); a NaN overlap, a non-positive ratio, a non-finite offset, a flip_x that is
 *            neither 0 nor 1; num_images other than the input's N; no merge open.
 *   _cascade_add   the same for the cascade deploys: blob triples and det_thr as in mscnn_net_detect_cascade_multi.
 *   _end     one synchronisation.  Output segment after segment: dets_host[cap][5] doubles, pass_host[cap] / row_host[cap] (may be
 *            NULL) = the forward (0-based add index) and the row of THAT forward's ROI blobs each detection came from, seg_dets[S],
 *            seg_candidates[S] (may be NULL) = candidates of each list.  Sort: larger prob first; a tie goes to the forward added
 *            first, inside a forward to the lower row.  More detections than cap is an error naming the numbers; a list that
 *            overflowed is an error naming the segment and the count.  The merge is closed afterwards, also when _end fails.
 *            Lists of more than 4032 slots run list after list on the tiled kernels, which take the default nms type / ovr_dnm only.
 * A _begin while a merge is open, and an _add or _end without _begin, are errors.  A stream-K hand-off time-out in one of the forwards
 * can not be answered by a re-run here: _end FAILS as mscnn_net_detect_end does, and the forwards are run and added again.
 * One forward added and merged is bit-identical to mscnn_net_detect_multi / mscnn_net_detect_cascade_multi.  No pin on the
 * reference: its scripts run one forward per image; the check is a numpy restatement (tests/merge_witness.py). */
#ifndef MSCNN_DETECTIONS_VIEW_DEFINED
#define MSCNN_DETECTIONS_VIEW_DEFINED
typedef struct { double off_x, off_y; int flip_x; } mscnn_detections_view;
#endif
MSCNN_NET_API int mscnn_net_detect_merge_begin(mscnn_net* net, int num_images, int num_classes, int cand_cap);
MSCNN_NET_API int mscnn_net_detect_merge_add(mscnn_net* net, const mscnn_detect_params* p, const mscnn_detections_view* view);
MSCNN_NET_API int mscnn_net_detect_cascade_merge_add(mscnn_net* net, const mscnn_detect_params* p, const mscnn_detections_view* view,
                                                     int num_outputs, const char* const* bbox_blobs, const char* const* prob_blobs,
                                                     const char* const* proposal_blobs, float det_thr);
MSCNN_NET_API int mscnn_net_detect_merge_end(mscnn_net* net, double* dets_host, int* pass_host, int* row_host, int cap, int* seg_dets,
                                             int* seg_candidates);
/* Box voting behind the merge (mscnn_hip.h: mscnn_detections_merge_vote_fwd): while it is on, mscnn_net_detect_merge_end enqueues the
 * vote between the merge and the one synchronisation, and every detection's box [x y w h] comes back as the prob-weighted mean of
 * the candidates of its list -- all forwards' -- whose union overlap with it is >= thr; prob, pass and row stay those of the kept
 * box, and a box with fewer than two voters comes back bit for bit.  Sticky, like mscnn_net_set_nms: thr = 0 is off (the default;
 * _end then enqueues exactly what it always did), any other value must lie inside (0, 1) or the call fails naming the value and
 * changes nothing.  Both calls work on a net built with device -1.  No pin on the reference: its scripts neither merge nor vote;
 * the check is tests/vote_witness.py (the op's documented summation order, bit for bit). */
MSCNN_NET_API int mscnn_net_set_box_voting(mscnn_net* net, double thr);
MSCNN_NET_API int mscnn_net_get_box_voting(const mscnn_net* net, double* thr);
/* Soft-NMS in place of the merge's hard NMS (mscnn_hip.h: mscnn_detections_merge_soft_fwd; Bodla et al., 2017): while it is on,
 * mscnn_net_detect_merge_end enqueues the soft op where it enqueued mscnn_detections_merge_fwd -- a candidate that overlaps a picked
 * box is not deleted, its score is decayed (method 1, linear: by 1 - IoU above the list's nms_overlap; method 2, gaussian: by
 * exp(-IoU^2 / sigma)) -- and every detection comes back with its decayed score, in pick order; candidates are picked until the best
 * live score is below score_thr or, with max_out > 0, max_out are out.  The sticky set_nms type / ovr_dnm are not read by the soft
 * op (the union form always; thr / det_thr were applied by the adds).  With box voting on, the vote runs behind it; the read-back is
 * unchanged.  Sticky, like mscnn_net_set_box_voting: method 0 is off (the default; _end then enqueues exactly what it always did; the
 * other three values are stored as given).  Refused, naming the value and changing nothing: a method outside {0, 1, 2}, gaussian
 * with a sigma that is not finite or not > 0, a score_thr that is NaN, infinite or < 0, max_out < 0.  Both calls work on a net built
 * with device -1.  No pin on the reference: its scripts neither merge nor decay a score; the check is tests/soft_witness.py. */
MSCNN_NET_API int mscnn_net_set_soft_nms(mscnn_net* net, int method, double sigma, double score_thr, int max_out);
MSCNN_NET_API int mscnn_net_get_soft_nms(const mscnn_net* net, int* method, double* sigma, double* score_thr, int* max_out);
/* Matrix NMS in place of the merge's hard NMS (mscnn_hip.h: mscnn_detections_merge_matrix_fwd; Wang et al., SOLOv2, 2020): while it
 * is on, mscnn_net_detect_merge_end calls the matrix op where it calls mscnn_detections_merge_fwd -- every candidate's score is
 * decayed by its worst overlap with a higher-ranked candidate, compensated by that candidate's own worst overlap (method 1, linear:
 * min (1 - IoU) / (1 - comp); method 2, gaussian: exp(-max (IoU^2 - comp^2) / sigma)), with no serial pick loop -- and the candidates
 * with score' >= score_thr come back in descending score' order, the first max_out of them when max_out > 0.  These are NOT
 * Soft-NMS's scores: a decay is the worst single pair, compensated, not a product over picks.  The segment's nms_overlap and the
 * sticky set_nms type / ovr_dnm are not read by the op (thr / det_thr were applied by the adds).  With box voting on, the vote runs
 * behind it; the read-back is unchanged.  Sticky: method 0 is off (the default; _end then enqueues exactly what it always did).
 * Matrix NMS and Soft-NMS exclude each other: turning one on while the other is on fails, naming both, and changes nothing.
 * Refused, naming the value and changing nothing: a method outside {0, 1, 2}, gaussian with a sigma that is not finite or not > 0,
 * a score_thr that is NaN, infinite or < 0, max_out < 0.  Both calls work on a net built with device -1.  No pin on the reference:
 * its scripts neither merge nor decay a score; the check is tests/matrix_witness.py.  The accuracy of Matrix NMS against Soft-NMS
 * was not evaluated (no labels here). */
MSCNN_NET_API int mscnn_net_set_matrix_nms(mscnn_net* net, int method, double sigma, double score_thr, int max_out);
MSCNN_NET_API int mscnn_net_get_matrix_nms(const mscnn_net* net, int* method, double* sigma, double* score_thr, int* max_out);
/* Weighted boxes fusion in place of the merge's hard NMS (mscnn_hip.h: mscnn_detections_merge_wbf_fwd; Solovyev, Wang, Gabruseva,
 * 2019 / 2021): while it is on, mscnn_net_detect_merge_end enqueues the WBF op where it enqueues mscnn_detections_merge_fwd -- the
 * candidates are walked in score order into clusters, a cluster's box is the score-weighted mean of all its members (and is what the
 * next candidate is matched against, union overlap > thr), its confidence the mean (conf_type 1, avg) or the largest (2, max) member
 * score times min(members, expected) / expected -- and the clusters come back in descending confidence, the first max_out of them
 * when max_out > 0; candidates with a score below skip_thr (or not > 0) do not enter.  The read-back is the one there is: pass / row
 * are those of the cluster's FIRST member.  expected = 0 means the number of views that were added to the frame's lists since _begin,
 * which the host counts per frame: + 1 per image for _add / _cascade_add, + 1 per b with list_of[b] == frame for the _views forms;
 * any other value >= 1 is used for every list.  The segment's nms_overlap and the sticky set_nms type / ovr_dnm are not read by the op
 * (thr / det_thr were applied by the adds).  Sticky: thr = 0 is off (the default; _end then enqueues exactly what it always did).
 * WBF, Soft-NMS, Matrix NMS and box voting exclude one another where WBF is one of the two (a vote behind a fusion would average
 * twice): turning one on while the other is on fails, naming both, and changes nothing.  Refused, naming the value and changing
 * nothing: a thr that is neither 0 nor inside (0, 1), a skip_thr that is NaN, infinite or < 0, a conf_type outside {1, 2},
 * expected < 0, max_out < 0.  Both calls work on a net built with device -1.
 * mscnn_net_detect_merge_members: after an _end that ran WBF, the member count of every detection that _end returned, segment after
 * segment in the order of dets_host (seg_dets[S] as _end filled it; cap = the ints members_host holds).  The counts came over with the
 * pack in that _end's one synchronisation.  It is an error, naming the reason, when the last _end did not run WBF (or failed).
 * No pin on the reference: its scripts neither merge nor fuse; the check is tests/wbf_witness.py.  The accuracy of WBF against the
 * hard merge, Soft-NMS and Matrix NMS was not evaluated (no labels here). */
MSCNN_NET_API int mscnn_net_set_wbf(mscnn_net* net, double thr, double skip_thr, int conf_type, int expected, int max_out);
MSCNN_NET_API int mscnn_net_get_wbf(const mscnn_net* net, double* thr, double* skip_thr, int* conf_type, int* expected, int* max_out);
MSCNN_NET_API int mscnn_net_detect_merge_members(mscnn_net* net, int* members_host, int cap, const int* seg_dets);
/* Seq-NMS over the frames of a clip in place of the merge's hard NMS (mscnn_hip.h: mscnn_detections_merge_seq_fwd; Han, Khorrami, Paine
 * et al., 2016).  While it is on, the lists of the open merge ARE the consecutive frames of one clip, in list order --
 * _begin(num_frames, K, cand_cap) is unchanged, num_frames <= 256 -- and mscnn_net_detect_merge_end enqueues the seq op where it
 * enqueues mscnn_detections_merge_fwd: per slot, the boxes of neighbouring frames whose union overlap is > link_thr are linked, the
 * chain of boxes with the largest score sum comes out with the chain's mean (rescore 1, avg) or largest (2, max) score on every box,
 * and suppresses what its boxes overlap by more than the segment's nms_overlap in their own frames; again until no box is left.  Of each
 * list the leading candidates with a score >= score_thr take part, at most top_k (<= 1024); the first max_out rows of a list come back
 * when max_out > 0.  The read-back, pass_host / row_host, the overflow error and the single synchronisation are unchanged.  The
 * frames' views still go to the frame's list (_add_views with list_of): the multi-view recipe and the clip recipe compose.  The
 * sticky set_nms type / ovr_dnm are not read by the op (thr / det_thr were applied by the adds).  Sticky: link_thr = 0 is off (the
 * default; _end then enqueues exactly what it always did).  Seq-NMS excludes Soft-NMS, Matrix NMS and WBF: turning one on while the
 * other is on fails, naming both, and changes nothing; box voting runs behind it as behind Soft-NMS and Matrix NMS.  Refused, naming
 * the value and changing nothing: a link_thr that is neither 0 nor inside (0, 1), a score_thr that is NaN, infinite or < 0, a top_k
 * outside [1, 1024], a rescore outside {1, 2}, max_out < 0; and, while it is on, a _begin with num_frames > 256 (nothing is opened) or an
 * _end of a merge begun with more (the setting was turned on behind _begin).  All three calls work on a net built with device -1.
 * mscnn_net_detect_merge_sequences: after an _end that ran Seq-NMS, the sequence id of every detection that _end returned, segment
 * after segment in the order of dets_host (seg_dets[S] as _end filled it; cap = the ints seq_host holds); an id is unique within a clip
 * and slot.  The ids came over with the pack in that _end's one synchronisation.  It is an error, naming the reason, when the last
 * _end did not run Seq-NMS or failed, at whatever point.
 * No pin on the reference: its scripts run one forward per image and look at no other frame; the check is tests/seq_witness.py.  The
 * accuracy of Seq-NMS was not evaluated (no labels here). */
MSCNN_NET_API int mscnn_net_set_seq_nms(mscnn_net* net, double link_thr, double score_thr, int top_k, int rescore, int max_out);
MSCNN_NET_API int mscnn_net_get_seq_nms(const mscnn_net* net, double* link_thr, double* score_thr, int* top_k, int* rescore, int* max_out);
MSCNN_NET_API int mscnn_net_detect_merge_sequences(mscnn_net* net, int* seq_host, int cap, const int* seg_dets);
/* Track ids across the frames of a stream (mscnn_hip.h: mscnn_tracks_update_fwd; BYTE association, Zhang et al., 2022, with a
 * constant-velocity prediction -- the paper's Kalman filter is there on request: mscnn_net_set_tracker_kalman below -- and a greedy
 * walk under a total order as the matching -- the optimal assignment SORT, DeepSORT and ByteTrack solve is there on request:
 * mscnn_net_set_tracker_assign below).
 * While the tracker is on, mscnn_net_detect_multi, mscnn_net_detect_cascade_multi and mscnn_net_detect_merge_end enqueue the update
 * behind their pack -- on _end behind whichever merge op is on, and behind the vote --, on the same stream, in front of the one
 * synchronisation those calls already have; the ids go behind the pack in the same pinned block, where WBF's member counts and (in
 * front of them) Seq-NMS's sequence ids go, and come over with it.  The detections those calls return are unchanged.  The images of
 * the call, or the frames (lists) of the merge, are consecutive frames of the stream in ascending order; a slot (class, or output x
 * class) has a table of at most max_tracks tracks of its own.  K, the slots per frame, is fixed by the first call after a reset; a
 * call with another K is refused, naming both values.
 * The Net keeps two tables: a call reads the committed one and writes the other, and they are swapped only after the call has
 * succeeded -- a call whose body runs twice (a stream-K hand-off recovery) or that fails steps the tracks neither twice nor half.
 * mscnn_net_set_tracker: params NULL = off (the default: no call does anything it did not do before, no allocation, no launch);
 * otherwise on with these values and a FRESH table (the next call starts at id 1).  Sticky.  Refused, naming the value and changing
 * nothing: everything mscnn_tracks_update_fwd refuses about params and max_tracks; and turning it on while weighted boxes fusion is
 * on, or set_wbf while it is on (the ids go where WBF's member counts go).  While it is on, the single-segment and the asynchronous
 * forms -- mscnn_net_detect, _detect_image, _detect_begin, _detect_device, _detect_multi_device, _detect_cascade,
 * _detect_cascade_multi_device -- are refused, naming the setting: no frame goes by untracked without a word.
 * mscnn_net_get_tracker: on (0 / 1), the values, and num_slots = the K the table was made for (0: not fixed yet).
 * mscnn_net_tracker_reset: a new stream -- the next call makes a fresh table (ids from 1) and fixes K again.
 * mscnn_net_detect_tracks: after a tracked call, the track id of every detection that call returned, segment after segment in the
 * order of dets_host (seg_dets[S] as the call filled it; cap = the ints ids_host holds); 0 = the detection belongs to no confirmed
 * track.  It is an error, naming the reason, when the last of the three calls did not run the tracker or failed.
 * mscnn_net_tracker_state: a host copy of the committed table (mscnn_tracks_state_layout_of(num_slots, max_tracks); bytes = what
 * state_host holds).  set / get / reset work on a net built with device -1.
 * No pin on the reference: its scripts run one forward per image and look at no other frame; the check is tests/track_witness.py.
 * The accuracy of the tracker was not evaluated (no labels here). */
#ifndef MSCNN_TRACK_PARAMS_DEFINED      /* include/mscnn_hip.h's struct, repeated here so that this header stands alone */
#define MSCNN_TRACK_PARAMS_DEFINED
typedef struct { double high_thr, low_thr, new_thr, match_thr, match_thr_low, vel_gain;
                 int motion, max_age, min_hits; } mscnn_track_params;
#endif
MSCNN_NET_API int mscnn_net_set_tracker(mscnn_net* net, const mscnn_track_params* params /* NULL: off */, int max_tracks);
MSCNN_NET_API int mscnn_net_get_tracker(const mscnn_net* net, int* on, mscnn_track_params* params, int* max_tracks, int* num_slots);
MSCNN_NET_API int mscnn_net_tracker_reset(mscnn_net* net);
MSCNN_NET_API int mscnn_net_detect_tracks(mscnn_net* net, int* ids_host, int cap, const int* seg_dets);
MSCNN_NET_API int mscnn_net_tracker_state(mscnn_net* net, void* state_host, size_t bytes);
/* The tracker for a batch of STREAMS (mscnn_hip.h: mscnn_tracks_update_streams_fwd): in live video a batch is one frame from each
 * of several cameras, and every camera needs a table of its own.
 * mscnn_net_set_tracker_streams: the frames of the tracked calls that follow belong to num_streams streams ([1, 256]).  It needs the
 * tracker on, gives a FRESH table and leaves K unfixed (as mscnn_net_tracker_reset), and clears the frame mapping.
 * mscnn_net_set_tracker puts it back to 1; with 1 every tracked call does exactly what it does without this call.
 * mscnn_net_set_frame_streams: the sticky mapping for the tracked calls that follow -- image b of mscnn_net_detect_multi and
 * mscnn_net_detect_cascade_multi, list f of mscnn_net_detect_merge_end, belongs to stream stream_of[b] resp. stream_of[f], inside
 * [0, num_streams).  The images (lists) of one stream are consecutive frames of it in ascending order; a stream may have none in a
 * call (nothing of it moves, no track of it ages).  NULL or count 0 clears it.  With num_streams > 1 a tracked call whose frame count
 * differs from count -- or that has no mapping -- is refused before its final stage is enqueued, naming both numbers.
 * mscnn_net_get_tracker_streams: num_streams, and the mapping (count entries into stream_of[cap]; count 0: none set).
 * mscnn_net_tracker_reset_stream: the K tables of stream s are reset on the committed table, on the net's stream, in front of the
 * next tracked call's update: that camera starts again at id 1, the others keep their tracks.  It succeeds and does nothing while K
 * is not fixed; an s outside [0, num_streams) is refused.  The two-table rule holds: a call whose body runs twice or that fails steps
 * nothing twice (a table reset twice is a table reset once).
 * mscnn_net_tracker_state copies num_streams * K tables, (stream s, slot k) at s * K + k; mscnn_net_detect_tracks is unchanged.
 * With num_streams > 1 Seq-NMS is refused in both directions, naming the setting: a clip links list t to list t - 1, so it is one
 * stream.  set / get / reset work on a net built with device -1.  No pin on the reference; the accuracy was not evaluated. */
MSCNN_NET_API int mscnn_net_set_tracker_streams(mscnn_net* net, int num_streams);
MSCNN_NET_API int mscnn_net_set_frame_streams(mscnn_net* net, const int* stream_of /* HOST, [count]; NULL: clear */, int count);
MSCNN_NET_API int mscnn_net_get_tracker_streams(const mscnn_net* net, int* num_streams, int* stream_of, int cap, int* count);
MSCNN_NET_API int mscnn_net_tracker_reset_stream(mscnn_net* net, int s);
/* A Kalman filter per track (mscnn_hip.h: mscnn_tracks_update_kalman_fwd, whose comment holds the steps): a second setting beside
 * the tracker's, so that mscnn_track_params and mscnn_net_set_tracker stay what they are.
 * mscnn_net_set_tracker_kalman: params NULL = off.  Otherwise it needs the tracker on with MSCNN_TRACK_MOTION_NONE (the filter is the
 * motion) and is refused otherwise, naming the motion; so is a std that is NaN, not finite or <= 0, naming it.  On, and off while
 * it was on, give a FRESH table and leave K unfixed, exactly as mscnn_net_set_tracker_streams does, and keep the number of streams
 * and the frame mapping; off while it is off changes nothing (the tracks live on).  mscnn_net_set_tracker turns the filter off, as it
 * puts the streams back to 1.
 * While it is on, every tracked call (mscnn_net_detect_multi, _detect_cascade_multi, _detect_merge_end) runs
 * mscnn_tracks_update_kalman_fwd in the place of mscnn_tracks_update_fwd / _streams_fwd.  There are two filter tables beside the two
 * track tables, swapped with them and only after success (the two-table rule).  mscnn_net_tracker_reset and _reset_stream work as
 * before: a filter table needs no reset, a record is made at its track's birth.  Everything else about those calls is unchanged: the
 * detections they return, where the ids land, mscnn_net_render and mscnn_net_crops behind them.
 * mscnn_net_get_tracker_kalman: on (0 / 1) and the values (the defaults while it has never been set).
 * mscnn_net_tracker_kalman_state: a host copy of the committed filter table, num_streams * K * max_tracks records of
 * mscnn_track_kalman_record beside the records of mscnn_net_tracker_state; refused, naming the reason, while the filter is off or K
 * is not fixed, and for a buffer that is too small.  set / get work on a net built with device -1.
 * The check is tests/track_kalman_witness.py; the accuracy was not evaluated (no labels here). */
#ifndef MSCNN_TRACK_KALMAN_PARAMS_DEFINED      /* include/mscnn_hip.h's struct, repeated here so that this header stands alone */
#define MSCNN_TRACK_KALMAN_PARAMS_DEFINED
typedef struct { double std_position, std_velocity;                              /* x h: 1/20, 1/160 */
                 double std_aspect, std_aspect_velocity, std_aspect_measure;     /* 1e-2, 1e-5, 1e-1 */
                 int freeze_lost_height; /* 1 */ } mscnn_track_kalman_params;
#endif
MSCNN_NET_API int mscnn_net_set_tracker_kalman(mscnn_net* net, const mscnn_track_kalman_params* params /* NULL: off */);
MSCNN_NET_API int mscnn_net_get_tracker_kalman(const mscnn_net* net, int* on, mscnn_track_kalman_params* params);
MSCNN_NET_API int mscnn_net_tracker_kalman_state(mscnn_net* net, void* filter_host, size_t bytes);
/* The matching of the tracker's two passes (mscnn_hip.h: mscnn_tracks_update_assign_fwd, whose comment holds steps 4'' and 5''):
 * method 1 (MSCNN_TRACK_ASSIGN_GREEDY, the default) is the walk by descending overlap, method 2 (MSCNN_TRACK_ASSIGN_OPTIMAL) the
 * maximum-weight assignment over the eligible pairs.
 * mscnn_net_set_tracker_assign needs the tracker on and refuses a method outside {1, 2}, naming it.  It touches NO table: both forms
 * read and write the same ones, so the next tracked call goes on from the committed tracks with the other matching; the streams, the
 * frame mapping and the Kalman filter stay as they are.  With method 2 every tracked call runs mscnn_tracks_update_assign_fwd in
 * the place of the op it ran before; with method 1 it runs exactly what it ran before this call existed.  mscnn_net_set_tracker puts it
 * back to 1, as it puts the streams back to 1.  Under method 2 header word 5 of a table (MSCNN_TRACKS_STEPS, in
 * mscnn_net_tracker_state's copy) is the table's running total of search steps; a call under method 1 writes 0 there.
 * mscnn_net_get_tracker_assign: the method, 0 while the tracker is off.  Both work on a net built with device -1.
 * The check is tests/track_assign_witness.py; the accuracy was not evaluated (no labels here). */
MSCNN_NET_API int mscnn_net_set_tracker_assign(mscnn_net* net, int method);
MSCNN_NET_API int mscnn_net_get_tracker_assign(const mscnn_net* net, int* method);
/* Draw the detections into the frames (mscnn_hip.h: mscnn_render_detections_u8, whose comment is the contract: footprints, paint
 * order, blend, labels, pixelation): the `show` block at the end of the reference's demo scripts, on the device.  It renders the pack
 * of the LAST mscnn_net_detect_multi, mscnn_net_detect_cascade_multi or mscnn_net_detect_merge_end on this net -- the Net still holds
 * it, as mscnn_net_detect_tracks reads that call's ids -- and, if that call ran the tracker, the tracker's id buffer.  frames_rgb: a
 * HOST array of count host pointers (device pointers when on_device != 0), frame b uint8 [org_h[b]][org_w[b]][3]: the frames that
 * call detected on, in its order (image b, or list b of the merge).  out_rgb: count host pointers (device pointers when
 * out_on_device != 0) to buffers of the same sizes, every byte of which is written; they must not overlap the frames or each other.
 * The pack (and the ids) go to a device buffer of the render stage's own in one copy, host frames are staged through buffers of its
 * own -- never through the buffer of mscnn_net_set_images, which may already hold the next forward's frames --, one launch per 32
 * frames on the net's stream; host outputs come back behind ONE synchronisation, device outputs are left asynchronous on that
 * stream.  It reads the pack and steps nothing: what mscnn_net_detect_tracks and mscnn_net_tracker_state return is unchanged.
 * Refused, naming the values: before any of the three calls has succeeded, or when another call that lands its result in the same
 * block (mscnn_net_detect, _detect_image, _detect_cascade, _proposals_multi, a failed call) has run since; a count that is not that
 * call's number of images or lists (both numbers); label >= 2 or color_by 1 when that call ran no tracker; a null frame; and
 * everything the op refuses.
 * NOT covered: the single-pack calls mscnn_net_detect and mscnn_net_detect_begin / _end (and the _device forms, whose pack the caller
 * owns: hand it to the op).  A batch of one through mscnn_net_detect_multi serves them. */
#ifndef MSCNN_RENDER_PARAMS_DEFINED      /* include/mscnn_hip.h's struct, repeated here so that this header stands alone */
#define MSCNN_RENDER_PARAMS_DEFINED
typedef struct {
  double show_thr;        /* a row with !(score >= show_thr) is not drawn (NaN: not drawn) */
  int thickness;          /* outline width in pixels, inwards from the box edge; 0: none; at most 64 */
  int outline_alpha;      /* 0 .. 256 */
  int fill_alpha;         /* 0 .. 256, the box's whole area under the outline; 0: none */
  int label;              /* 0 none, 1 score, 2 track id, 3 id and score */
  int label_scale;        /* integer glyph magnification, 1 .. 8 */
  int color_by;           /* 0: the slot (class / output x class), 1: the track id */
  int pixelate;           /* 0 off, else the mosaic block edge, 2 .. 64 */
  int num_colors;         /* 1 .. 32 */
  unsigned char colors[32][3];   /* RGB */
} mscnn_render_params;
#endif
MSCNN_NET_API int mscnn_net_render(mscnn_net* net, const unsigned char* const* frames_rgb, int on_device,
                                   const int* org_h, const int* org_w, int count, const mscnn_render_params* p,
                                   unsigned char* const* out_rgb, int out_on_device);
/* Every detection as a fixed-size, mean-subtracted patch, cut on the device: what a second stage -- a re-identification or attribute
 * net, a face recogniser, a gallery of a track's sightings -- takes from a detector.  It reads the pack mscnn_net_render reads: the
 * block the LAST successful mscnn_net_detect_multi, mscnn_net_detect_cascade_multi or mscnn_net_detect_merge_end left, with the
 * tracker's ids behind it if that call ran the tracker; the same validity record (any other user of the block ends it) and the same
 * rule for a segment's rows (entry {count, rows, row0, 0}; offset = row0, unless K >= 2 and the entries of the frame's slots 0 and 1
 * hold the same row0, then K * row0 + k * rows; a segment with count < 0, a negative offset or offset + count > cap is empty).  It
 * reads the pack and steps nothing: mscnn_net_detect_tracks, mscnn_net_tracker_state and a following mscnn_net_render are unchanged,
 * and render and crops may both follow one detect call, in either order.
 * No new device op: the pixels are mscnn_preprocess_views_u8_f32's (mscnn_hip.h), one call over all windows; the host computes the
 * windows.  frames_rgb / on_device / org_h / org_w / count: as mscnn_net_render -- the frames that call detected on, in its order.
 * The window of a row [x y w h s] in a frame of org_h x org_w.  Double arithmetic, one rounding per operation (no fused
 * multiply-add), up to the four floors of step 4; from there on integers only, in 64 bits:
 *   1. The row is SKIPPED when !(s >= thr); when one of its five values is not finite; when !(w > 0) or !(h > 0); when |x|, |y|, w or
 *      h exceeds 2^30.
 *   2. ww = w * context;  hh = h * context.
 *   3. With fit == 1:  a = (double)out_w / (double)out_h;  t = hh * a;  if ww < t then ww = t, else hh = ww / a.
 *   4. cx = x + w / 2;  cy = y + h / 2;  x0 = cx - ww / 2;  y0 = cy - hh / 2;  and, in the footprint rounding of the render stage,
 *      L = floor(x0 + .5), T = floor(y0 + .5), R = floor((x0 + ww) + .5) - 1, B = floor((y0 + hh) + .5) - 1;
 *      Wd = R - L + 1, Ht = B - T + 1.  The row is skipped when Wd < 1 or Ht < 1.
 *   5. With border == 1 (shift; as mscnn_amd.net.tile_views: a window that fits is moved inwards, not shrunk), horizontally:
 *      if Wd >= org_w then L = 0, Wd = org_w; else if L < 0 then L = 0; else if L + Wd > org_w then L = org_w - Wd.  Vertically the
 *      same with T, Ht, org_h.
 *   6. With border == 0 (clip): L' = max(L, 0), R' = min(R, org_w - 1), T' = max(T, 0), B' = min(B, org_h - 1).  The row is skipped
 *      when the clipped window is empty (L' > R' or T' > B'); otherwise the window is the clipped one.
 *   7. The row is skipped when Wd < min_size or Ht < min_size.
 *   The window is {x0 = L, y0 = T, w = Wd, h = Ht} and lies inside the frame.
 * Order and bound.  Crops come out in the order (frame, slot, row), each ascending; row 0 of a segment is its best score.  The slot
 * filter and tracked_only (a row's track id > 0) apply before counting; the first max_crops rows in that order that give a crop are
 * produced, *num_dropped = the further rows that would have given one (the call succeeds: a drop is never silent).  *num_crops may
 * be 0; nothing is uploaded or launched then.
 * Pixels.  out: [max_crops][3][out_h][out_w] floats in host memory, or in device memory when out_on_device != 0.  Slices
 * [0, *num_crops) are written, later slices are left as they were.  Slice i is what the views op defines: bit-identical to
 * mscnn_preprocess_u8_f32 on a contiguous copy of the window -- the scripts' imresize to out_h x out_w, planes B, G, R, mean_bgr
 * subtracted per plane.  info_host[max_crops] (host): entry i = where crop i came from (row: its index inside its segment;
 * track_id: 0 when that call ran no tracker) and its window in frame pixels; complete when the call returns, whatever out is.
 * How it runs.  One mscnn_preprocess_views_u8_f32 call over all windows on the net's stream, its workspace
 * (mscnn_preprocess_views_workspace_bytes) kept with the Net and grown when needed.  A host frame is uploaded once, whatever the
 * number of its crops, and not at all when it has none.  Staging goes through buffers of this stage's own -- never through the buffer
 * of mscnn_net_set_images, which may already hold the next forward's frames.  A device out is left asynchronous on the net's stream;
 * a host out comes back behind ONE synchronisation.
 * Refused before anything is uploaded or enqueued, naming the value: a null pointer; no valid pack (render's text, starting
 * "crops:"); a count that is not that call's number of images or lists (both numbers); a null frame, a frame size <= 0 or above
 * 2^30; a NaN thr; context outside [1, 16] (NaN included); fit or border outside {0, 1}; min_size < 1; out_h or out_w outside
 * [1, 1024]; max_crops < 1; slot outside [-1, slots of that call); tracked_only outside {0, 1}, or 1 when that call ran no tracker; a
 * mean that is not finite; a net built with device < 0.
 * mscnn_net_crop_window: steps 1 - 7 for one row on the host -- no device, no net; it is the function mscnn_net_crops itself calls
 * per row.  Returns 1 and win = {x0, y0, w, h} when the row gives a crop, 0 when it is skipped, < 0 (the text in
 * mscnn_net_last_error) for params mscnn_net_crops would refuse -- of slot only "below -1" can be told here --, a null pointer or a
 * frame size <= 0 or above 2^30.
 * NOT covered, as for mscnn_net_render: the single-pack calls; a batch of one through mscnn_net_detect_multi serves them.  No uint8 /
 * HWC patches, no padding of a window that leaves the frame, no rotation.
 * No pin on the reference: its scripts cut no patches.  The windows' check is tests/crops_witness.py, a restatement of the rule
 * above in plain Python numbers; the pixels' check is the single-frame op on a host copy of the window. */
typedef struct {
  double thr;          /* a row with !(score >= thr) gives no crop (NaN thr: refused) */
  double context;      /* the window is the box scaled about its centre by this factor; 1 <= context <= 16 (MS-CNN's own ROI context is 1.5) */
  int fit;             /* 0: the scaled box as it is (stretched to out_h x out_w); 1: grown to the aspect ratio out_w : out_h first */
  int border;          /* 0: the window is clipped to the frame; 1: a window that fits is shifted inwards, not shrunk (as net.tile_views) */
  int min_size;        /* >= 1: a window narrower or lower than this, after step 6, gives no crop */
  int out_h, out_w;    /* 1 .. 1024 */
  int max_crops;       /* >= 1: rows of `out` and of `info` */
  int slot;            /* -1: every slot; else only this one, inside [0, slots of that call) */
  int tracked_only;    /* 1: only rows whose track id is > 0 (needs a call that ran the tracker) */
  float mean_bgr[3];   /* subtracted per plane; {0, 0, 0} gives the resized pixel values themselves */
} mscnn_crops_params;
typedef struct { int frame, slot, row, track_id; int x0, y0, w, h; } mscnn_crop_info;   /* row: index inside its segment; the window in frame pixels */
MSCNN_NET_API int mscnn_net_crop_window(const mscnn_crops_params* p, const double row[5], int org_h, int org_w, int win[4]);
MSCNN_NET_API int mscnn_net_crops(mscnn_net* net, const unsigned char* const* frames_rgb, int on_device, const int* org_h, const int* org_w,
                                  int count, const mscnn_crops_params* p, float* out, int out_on_device,
                                  mscnn_crop_info* info_host, int* num_crops, int* num_dropped);
/* The views of a frame as ONE batched forward (mscnn_hip.h: mscnn_detections_candidates_add_views): the merge was opened with
 * _begin(num_frames, ...), the input holds N images -- the views mscnn_net_set_image_views wrote --, p[N * K] and view[N] describe
 * them as in _add, and list_of[N] (host) names the frame of each: the rows of image b go to the lists of frame list_of[b].  One
 * call is ONE pass (the tag's row is absolute in the batch).  Order of a list: (add call, image index ascending, row), whatever the
 * timing.  Refused before anything is enqueued, naming the value: everything _add refuses but its num_images rule, a null list_of,
 * an entry outside [0, num_frames).  The row bound (the sum of the forwards' ROI row counts against cand_cap) applies unchanged; the
 * nms_overlap rule is per LIST: every image that reaches a list, in this call or an earlier one, carries the overlap the list got
 * first.  _end and its reader are unchanged.  No pin on the reference: its scripts have neither views nor a merge; the check is
 * tests/merge_witness.py with the passes listed in (add, image) order. */
MSCNN_NET_API int mscnn_net_detect_merge_add_views(mscnn_net* net, const mscnn_detect_params* p, const mscnn_detections_view* view,
                                                   const int* list_of);
MSCNN_NET_API int mscnn_net_detect_cascade_merge_add_views(mscnn_net* net, const mscnn_detect_params* p, const mscnn_detections_view* view,
                                                           const int* list_of, int num_outputs, const char* const* bbox_blobs,
                                                           const char* const* prob_blobs, const char* const* proposal_blobs, float det_thr);

/* Multi-GPU form of the same stage (include/mscnn_dist.h gathers its result over RCCL): the detections stay in HBM, in a
 * fixed-size pack  [int32 count, int32 num_rois, int32 cap, int32 0][cap x 5 doubles x y w h prob][cap x int32 roi row]
 * of mscnn_net_detect_pack_bytes(cap) bytes (a multiple of 16).  cap must be >= the net's ROI count (BoxOutput's
 * max_nms_num bounds it); more ROIs than cap is an error, never a truncation.  Asynchronous on the net's stream;
 * *pack_dev stays valid until the next detect call on this net.  mscnn_net_unpack_detections reads one pack on the host. */
MSCNN_NET_API size_t mscnn_net_detect_pack_bytes(int cap);
MSCNN_NET_API int mscnn_net_detect_device(mscnn_net* net, const mscnn_detect_params* p, int cap, const void** pack_dev);
MSCNN_NET_API int mscnn_net_unpack_detections(const void* pack_host, int cap, double* dets_host, int* ids_host, int* num_dets,
                                              int* num_rois);

#ifdef __cplusplus
}
#endif
#endif
