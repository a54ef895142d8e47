/*
 * mscnn_hip.h -- C ABI of libmscnn_hip.so: the MI355X (gfx950) device ops of the MS-CNN
 * inference hot path.  This is the drop-in boundary: every entry point is
 * what a caffe::Layer<float>::Forward_gpu of the reference would bind for that layer.
 * Plain pointers and sizes only; all tensors are fp32, NCHW, contiguous (blob.hpp:153-164);
 * every pointer is a DEVICE pointer unless the parameter name ends in _host.
 * `stream` is a hipStream_t passed as void* (NULL = the default stream, which is what every
 * reference layer uses, device_alternate.hpp:84-90).
 *
 * Return value: 0 = ok, non-zero = error (see mscnn_status).  Nothing here aborts; the C++
 * layer shim (mscnn_amd/host) turns a non-zero status into a CHECK-style fatal to mimic the
 * reference's glog convention (device_alternate.hpp:48-67).
 *
 * There is NO CPU fallback behind any of these functions.
 *
 * BUFFER CONTRACT (tests/test_gpu_buffer_contract.py holds every op to it, between guard bands and on poisoned memory):
 * workspaces and outputs may hold anything on entry -- an op initialises, on its own stream, every word it later reads, and
 * writes every element of its output (exceptions are stated at the op: pack rows past a slot's count, rows past count_out);
 * no op writes outside [p, p + bytes) of any buffer, where bytes is the tensor's size or what the op's *_bytes() query
 * returned, and none reads outside its inputs; no op writes through a const pointer.  Nothing waits on workspace contents of an
 * earlier call (the stream-K hand-off flags of the plane GEMM are tagged per launch and polled a bounded number of times).
 *
 * STREAM CONTRACT (tests/test_gpu_stream_contract.py holds every op to it behind a gate on a non-blocking side stream;
 * tests/test_stream_cases_cpu.py holds the list of ops against this header):
 * 1. Ordering.  An op enqueues ALL of its device work on `stream`: every launch, hipMemsetAsync and copy, and the profiling events
 *    of mscnn_conv2d_plan_set_profiling.  It reads its inputs, and writes its outputs and workspaces, only in stream order between
 *    the call and the next thing the caller enqueues on `stream`: what `stream` wrote before the call is seen, and the caller may
 *    overwrite an input or a workspace on `stream` as soon as the call has returned.  No op reads device memory from the host;
 *    *_host arrays and descriptor structs are read before the call returns and may be freed then.
 * 2. Asynchrony.  An op returns without waiting for `stream` or for the device.  Exceptions, all of them a first call of a kind:
 *      mscnn_inner_product_fwd_f32 / _f16 on the MFMA GEMM path   the library's slab buffer of (thread, device, stream) is made or grown
 *                                 with hipMalloc, behind a hipFree that waits for the device; a fifth stream on one thread takes over
 *                                 the least recently used of four buffers the same way (below)
 *      the plane GEMM with split tiles (Winograd wgemm plans, mscnn_inner_product_wg_fwd)   the process's hand-off word of the
 *                                 device, one hipHostMalloc at the first such launch on it
 *    and by its purpose mscnn_conv2d_plan_stage_ms, which waits for the plan's own events (hipEventSynchronize).  Plan creation,
 *    mscnn_conv2d_plan_set_batch and mscnn_conv2d_plan_destroy are host work and touch no stream; the events of a profiled plan are
 *    created by mscnn_conv2d_plan_set_profiling.
 * 3. Concurrency.  Calls on different streams may be in flight at once, from one host thread or several, where their caller-owned
 *    buffers are disjoint: outputs, workspace, packed weights being written, candidate buffer, pack, track state.  Inputs may be shared.
 *      - A plan belongs to one call in flight at a time (mscnn_conv2d_plan_set_batch, _set_amax_io and the profiling events change
 *        it), and so does a workspace, a candidate buffer, a pack and a track state.
 *      - The stream-K slabs of mscnn_inner_product_fwd_f32 / _f16 are the library's: one buffer per (host thread, device, stream),
 *        up to four streams per thread and device without a wait; calls on one stream share a buffer and are ordered by the stream.
 *      - The persistent-grid plane GEMM with split tiles (wgemm plans, mscnn_inner_product_wg_fwd) needs its workgroups co-resident:
 *        another stream's kernels can starve them, and then a launch may raise a hand-off event (mscnn_wgemm_handoff_event below) --
 *        reported, never silent.  mscnn_wgemm_force_whole_tiles(1) takes the precondition away.
 *      - mscnn_wgemm_force_whole_tiles, the mscnn_debug_* knobs and the hand-off event counter are per process, mscnn_last_error is
 *        per thread: none of them is per stream.
 *      - mscnn_sum_squares_f32 adds its partial sums with f64 atomics in the order the waves finish: its result is reproducible to
 *        rounding, not to the bit, on any stream.  Every other op gives the same bits on every stream.
 *
 * ALIGNMENT.  hipMalloc's 256 bytes satisfy every op.  Tighter than that, every pointer is in one of three classes: it needs only
 * its element type's own alignment (4 bytes for a float blob; "4" below); the op FALLS BACK to a slower kernel with the same result;
 * or the op REFUSES it with MSCNN_ERR_BAD_ARG before its first launch, so that nothing is stored through it and no workspace is touched.
 *   every op                   workspaces, packed weights (packed, wt, w16), prepared_maps, pack_dev: 16, refuses
 *   conv2d_fwd / _fwd_pool / _fwd_chain / _fwd_roipool_pair, by the plan's kernel (mscnn_conv2d_plan_kernel); w, bias, y_pool 4
 *     igemm_* (direct, ROI mode), igemm16_*, head4x4_*, head_kwfold_*, wconv_64x512_k3x3, direct_f32     x, y 4
 *     igemm16x3_* (split-fp16 direct)   y 4; x 16 for its max |x| pass, refuses (x 4 where in_bound hands max |x| over)
 *     igemm_*_vec (a 1x1 layer on 128-pixel rows), head_gemm_shiftadd_f32 on such rows                                 x 16: refuses
 *     conv3x3_c3_valu_f32        x, y 16: refuses
 *     winograd2x2_fused_k3x3_c64 x 16, y 8: refuses
 *     winograd_f4x4_3x3          x 16, y 16, y_pool 8: falls back to its scalar transforms; _fwd_chain with a next plan: y 16, refuses
 *     winograd_f3x3_3x3          x, y 4 on whole planes; on maps of <= 64 pixels x 16, y 16: falls back (scalar staging);
 *                                with y_pool: y 8 where Wo is even, refuses
 *     winograd_f2x2_3x3          x 4; y 8 where Wo is even: refuses
 *     winograd_f3x3_3x3_x3f16_*, head_gemm_shiftadd_x3f16   x 16 (the max |x| pass), refuses; y as winograd_f3x3_3x3
 *   conv2d_pack_weights        w 4; for a split-fp16 plan w 16 (the max |w| pass): refuses
 *   roipool_maps_build         feat 4
 *   relu_fwd                   4; the float4 kernel runs when x, y are 16-byte aligned and count % 4 == 0: falls back
 *   pool2d_fwd                 4; the 2x2 / stride 2 fast path needs x 16, y 8: falls back
 *   inner_product_fwd_f32      4; the MFMA GEMM (N >= 64) needs x, w 16 and K % 4 == 0: falls back to the row-wise / generic kernel
 *   inner_product_fwd_f16      x 16: refuses; y, bias 4
 *   inner_product_x3_fwd / _pack   x resp. w 16: refuses; y, bias 4
 *   inner_product_wg_fwd       x 16: refuses; y, bias 4; _wg_pack: w 4
 *   deconv_depthwise_fwd       4; the 4x4 / stride 2 / pad 1 quad kernel needs y 8: falls back to the per-output kernel
 *   concat_channels, softmax, eltwise, deconv2d (generic), roipool, roipool_pair, roialign, roialign_ave, roialign_ave_pair, decodebbox, preprocess* (images, out),
 *   max_rel_diff*, sum_squares, store_words      4 (doubles 8)
 *   nms_greedy                 boxes 16: refuses; keep_out 1
 *   boxoutput*                 heads, rois_out, props_out, anchor_ids_out, count_out_dev 4
 *   detections*                blobs, ids_out, count_out_dev 4; dets_out 8: refuses
 *   detections_candidates_*, detections_merge_fwd   cand, workspace, pack_dev 16: refuses; the blobs 4
 *   detections_merge_vote_fwd  cand, pack_dev 16: refuses
 *   detections_merge_soft_fwd  cand, workspace, pack_dev 16: refuses
 *   detections_merge_matrix_fwd  cand, workspace, pack_dev 16: refuses
 *   detections_merge_wbf_fwd   cand, workspace, pack_dev 16, members_dev 4: refuses
 *   detections_merge_seq_fwd   cand, workspace, pack_dev 16, seq_dev 4: refuses
 *   tracks_update_fwd, tracks_update_streams_fwd, tracks_state_reset, tracks_state_reset_slots
 *                              pack_dev, state_in, state_out (state) 16, track_ids_dev 4: refuses
 *   tracks_update_kalman_fwd   pack_dev, state_in, state_out, filter_in, filter_out 16, track_ids_dev 4: refuses
 *   tracks_update_assign_fwd   as tracks_update_kalman_fwd (the filter tables only with a filter): refuses
 *   proposals_multi_fwd        props 8: refuses
 *   rois_ingest                rows 8: refuses; rois, props, image_rows, status 4
 */
#ifndef MSCNN_HIP_H_
#define MSCNN_HIP_H_

#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__)
#define MSCNN_API __attribute__((visibility("default")))
#else
#define MSCNN_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  MSCNN_OK = 0,
  MSCNN_ERR_BAD_ARG = 1,      /* shape / parameter the kernel cannot honour */
  MSCNN_ERR_HIP = 2,          /* a HIP runtime call or launch failed; see mscnn_last_error() */
  MSCNN_ERR_WORKSPACE = 3,    /* workspace too small; query the *_workspace_bytes function */
  MSCNN_ERR_UNSUPPORTED = 4
} mscnn_status;

/* Text of the last error on this host thread (static storage, never NULL). */
MSCNN_API const char* mscnn_last_error(void);
/* Library / device identification: "mscnn_hip <ver> gfx950". */
MSCNN_API const char* mscnn_version(void);

/* ------------------------------------------------------------------------------------------
 * Convolution  -- replaces ConvolutionLayer<Dtype>::Forward_gpu (src/caffe/layers/conv_layer.cu:8-23
 * -> base_conv_layer.cpp:325-349: im2col_gpu + cublasSgemm + bias GEMM) and
 * CuDNNConvolutionLayer::Forward_gpu (cudnn_conv_layer.cu:11-46), fused with the in-place
 * ReLULayer::Forward_gpu that follows it in every deploy net (relu_layer.cu:17-26) when relu != 0.
 * Cross-correlation, weights w[Cout][Cin/group][Kh][Kw] (base_conv_layer.cpp:135-140), bias may be NULL.
 *
 * The hot shapes (stride 1, group 1) run on an im2col-free implicit-GEMM MFMA kernel that reads a
 * pre-packed copy of the weights: create a plan once per layer (weights are constants at inference),
 * call mscnn_conv2d_pack_weights whenever the Caffe weight blob changes, then mscnn_conv2d_fwd_f32.
 * ------------------------------------------------------------------------------------------ */
typedef struct mscnn_conv_plan mscnn_conv_plan;   /* opaque */

typedef enum {
  /* The default.  3x3 / stride 1 / group 1 layers with enough arithmetic intensity run a Winograd form: F(4x4,3x3) (36 planes, points
   * {0, 1, -1, 2, -1/2, inf}) where the layer has >= 1000 tiles of 4x4 (conv2_1 .. conv4_3, loss1_conv1 of the 7s-576 net), F(3x3,3x3)
   * (25 planes) below that and on 7x7 ROI maps (conv5_x, conv6_1, roi_c1); the plane GEMMs run on wgemm.hip's kernel.  Cin = 3 runs a
   * VALU kernel, Cout <= 16 with 5x5 / 7x7 / 3x5 / 5x7 kernels the M = 4 head kernels (or the kw-folded GEMM), a 3x3 / pad 1 layer with
   * 64 output channels on a full-resolution map (conv1_2: whole 4 x 128 tiles, >= 2 per CU) the ring kernel of wconv.hip, everything
   * else the direct implicit-GEMM kernel.  The Winograd forms carry ~10x the rounding error of the direct sum: callers that go through the
   * C++ layer (libmscnn_caffe.so) get a per-layer check against DIRECT on the first forward after every weight change, and a
   * fall-back, without asking (include/mscnn_net.h: mscnn_net_set_auto_calibrate); callers of THIS ABI own that decision and can
   * make it with mscnn_max_rel_diff_f32 on a DIRECT plan's output. */
  MSCNN_CONV_ALGO_AUTO = 0,
  MSCNN_CONV_ALGO_DIRECT = 1,   /* never Winograd: the k-ordered implicit-GEMM sum (per-layer numerical fall-back) */
  MSCNN_CONV_ALGO_WINO_F2 = 2,  /* F(2x2,3x3) on whole planes wherever it is legal (small ROI maps: F(3x3,3x3)) */
  MSCNN_CONV_ALGO_WINO_F3 = 3,  /* F(3x3,3x3) wherever it is legal */
  /* Reduced-precision mode (no reference counterpart): operands rounded to fp16 on their way into LDS, v_mfma_f32_32x32x16_f16
   * with fp32 accumulators, direct 3x3 implicit GEMM (no Winograd).  Blobs stay fp32.  Shapes without an fp16 kernel (stride,
   * groups, heads) run their fp32 kernel.  Tolerance policy: DESIGN.md (per-layer 5e-3 of the layer's scale; detections IoU >=
   * 0.95 and |dscore| <= 5e-3 against the fp32 path). */
  MSCNN_CONV_ALGO_F16 = 4,
  /* F(3x3,3x3) whose 25 plane GEMMs run on the fp16 MFMA pipe with every fp32 operand split exactly into two fp16 halves
   * (x s = hi + lo, s a power of two taken from the tensor's max |x|, measured on the device each forward) and three products
   * per pair, fp32 accumulators: 22-bit significands -- fp32-grade results (same 1e-4 parity bar as the fp32 kernels) at 16/3
   * of the fp32 MFMA rate.  Opt-in; it replaces the plane GEMMs of the layers the AUTO heuristic runs as F(3x3,3x3); every other
   * layer (and Cin not a multiple of 32) keeps its fp32 kernel.  mscnn_conv2d_plan_dtype() reports "f16x3". */
  MSCNN_CONV_ALGO_WINO_F3_X3 = 5,
  /* F(4x4,3x3) with the interpolation points {0, 1, -1, 2, -1/2, inf} wherever it is legal (whole planes; ROI maps keep
   * F(3x3,3x3)): 36 multiplies per 16 outputs, fp32 error 0.8 .. 3.2x (median 1.2x) the F(3x3,3x3) form's over 36 input / filter
   * distributions (profiles/r03_robustness.txt).  In production since round 3: AUTO selects it for the nine largest 3x3 layers of
   * the 7s-576 net (A/B per layer: profiles/r03_ab_wino_f4.txt); this value forces it also where AUTO would keep F(3x3,3x3). */
  MSCNN_CONV_ALGO_WINO_F4 = 6
} mscnn_conv_algo;

typedef struct {
  int N, Cin, H, W;          /* bottom shape */
  int Cout, Kh, Kw;
  int pad_h, pad_w, stride_h, stride_w, group;
  int relu;                  /* 1: apply max(x,0) in the epilogue (negative_slope 0) */
  int algo;                  /* mscnn_conv_algo; shapes an algorithm does not cover fall back to the direct kernels */
  /* Tuning knobs for A/B measurements (tools/bench_layers.py); 0 = the measured default.  None changes results beyond
   * fp32 rounding.  tune_variant: igemm tile variant (value + 1, so that 0 keeps the default); tune_grid: workgroups of the
   * persistent igemm / head kernels; tune_flags: bit 0 = no XCD-aware workgroup map, bit 1 = proposal heads on the 32-row
   * igemm tile instead of the M = 4 head kernel, bit 2 = MSCNN_CONV_ALGO_WINO_F3_X3 wherever it is legal (default: only where
   * the AUTO heuristic picks F(3x3,3x3)), bit 4 = fp32 proposal heads as one GEMM over the taps + shift-and-add (measured equal or
   * slower than the head kernel: opt-in), bit 5 = never that form, bit 6 = AUTO keeps F(3x3,3x3) where it would take F(4x4,3x3),
   * bit 7 = the Winograd plane GEMMs on the round-2 igemm kernel instead of wgemm.hip's, bit 8 = the scalar (host-checked)
   * F(4x4,3x3) transform kernels instead of the vectorised ones and the generic F(3x3,3x3) output transform on ROI maps instead of the LDS-staged one, bit 9 = never / bit 10 = wherever legal: proposal heads with the
   * kernel's columns folded into M (KH x 1 convolution with KW * Cout channels + shift-and-add), bit 11 = a Cin = 3 layer (conv1_1) on the MFMA igemm kernel instead of its VALU kernel, bit 12 = F(4x4,3x3) input transform with one tile per lane instead of two, bit 15 = a 3x3 / pad 1 layer with 64 output channels on whole 4 x 128 tiles (conv1_2) stays on the igemm kernel instead of the ring kernel of wconv.hip (bit-identical for whole tiles; A/B, second witness), bit 16 = (round 5) a 3x3 / pad 1 layer with 64 output channels on a full-resolution map (conv1_2: whole 8 x 32 blocks, >= 512 of them) stays on the direct ring kernel of wconv.hip instead of the one-launch Winograd F(2x2,3x3) kernel of wf2conv.hip that AUTO takes there (A/B, the direct witness; tune_variant 403 also plans smaller maps on it: tests), bit 14 = inverts the wave priority of the direct MFMA kernel's tile epilogue (raised by default on the 64 x 256 3x3 tile = conv1_2 only), bit 13 = (witness build only, `make -C mscnn_amd/csrc witness`; ignored by the product library) proposal heads on the packed-FMA kernel of tools/micro/headvalu.hip instead of the M = 4 MFMA kernel (headconv.hip), bit 17 = a small-map F(3x3,3x3) plan whose planes would be ragged (mscnn_conv2d_plan_plane_columns) keeps uniform planes (A/B; bit-identical under whole tiles); tune_variant with WINO_F3_X3: 1 = 128-row, 2 = 256-row GEMM tiles;
   * tune_variant 300 + v with a Winograd algo: wgemm tile variant v (1: 256 x 128, 2: 128 x 256, 3: 128 x 128, 4: 256 x 96, 5: 256 x 160; + 256 forces the
   * stream-K split, + 512 whole tiles).  Proposal heads (headconv.hip, round 5): tune_variant 500 / 501 = full / half channel chunks
   * whatever the map (AUTO: half chunks on maps of <= 16 tiles of 16 x 32 pixels and for the 5-row kernels everywhere); tune_grid > 0 = that many workgroups, clamped to the
   * number of (tile, chunk) units. */
  int tune_variant, tune_grid, tune_flags;
} mscnn_conv_desc;

MSCNN_API int mscnn_conv2d_plan_create(const mscnn_conv_desc* desc, mscnn_conv_plan** plan_out);
MSCNN_API void mscnn_conv2d_plan_destroy(mscnn_conv_plan* plan);
/* Bytes of device memory the plan needs for packed weights and for split-K partial tiles. */
MSCNN_API size_t mscnn_conv2d_packed_weight_bytes(const mscnn_conv_plan* plan);
MSCNN_API size_t mscnn_conv2d_workspace_bytes(const mscnn_conv_plan* plan);
/* Which kernel family the plan selected (static string):
 *   "winograd_f4x4_3x3" | "winograd_f3x3_3x3" | "winograd_f2x2_3x3"        input transform -> wgemm plane GEMM -> output transform
 *   "winograd_f3x3_3x3_x3f16_128" | "..._256"                               the same with split-fp16 plane GEMMs (WINO_F3_X3)
 *   "igemm_<BM>x<BN>_k3x3_..." | "igemm_<BM>x<BN>_k1x1_..."                 direct implicit GEMM on v_mfma_f32_32x32x2_f32
 *   "igemm16_..." | "igemm16x3_..."                                          the same on fp16 / split-fp16 operands
 *   "conv3x3_c3_valu_f32"                                                    Cin = 3 (conv1_1)
 *   "winograd2x2_fused_k3x3_c64" (conv1_2 on full-resolution maps: ONE launch -- input transform, 16 plane products on v_mfma_f32_16x16x4_f32,
 *                               output transform, ReLU and the 2x2 pooling inside a workgroup; executed FLOPs = 16 / 36 of the direct count)
 *   "wconv_64x512_k3x3" (the same shape class as a direct convolution: DIRECT, or tune_flags bit 16) | "head4x4_k<Kh>x<Kw>_m<..>" | "head_kwfold_shiftadd_f32" | "head_gemm_shiftadd_f32" | "head_gemm_shiftadd_x3f16"   proposal heads
 *   "direct_f32"                                                             any stride / group / kernel size (generic kernel)
 * A name that starts with "winograd" is what the numerical checks of the C++ layer key on. */
MSCNN_API const char* mscnn_conv2d_plan_kernel(const mscnn_conv_plan* plan);
/* Algorithmic FLOPs (2*MACs of the direct convolution the reference computes) of one forward call. */
MSCNN_API double mscnn_conv2d_plan_flops(const mscnn_conv_plan* plan);
/* "f32" | "f16" | "f16x3": the arithmetic type of the plan's MFMA operands (accumulation is fp32 in all of them). */
MSCNN_API const char* mscnn_conv2d_plan_dtype(const mscnn_conv_plan* plan);
/* FLOPs the MFMA pipe really executes for the real (unpadded) problem: equal to the algorithmic count for the direct
 * kernels, 2 * planes * Cout * Cin * tiles for the Winograd forms (25/81 resp. 16/36 of it on exactly tiled planes);
 * 2 * Cout * Cin * (sum of the planes' columns) where the planes are ragged. */
MSCNN_API double mscnn_conv2d_plan_executed_flops(const mscnn_conv_plan* plan);
/* Live GEMM columns of each transform plane of a Winograd plan: cols[p], p < min(n, planes); returns the number of planes (0: not
 * a Winograd plan).  N * tiles_h * tiles_w for every plane, except on a ragged plan: a small-map (H * W <= 64) fp32 F(3x3,3x3)
 * plan on the wgemm kernel, without a pooled output, whose output is no whole number of 3 x 3 tiles.  There plane (i, j) has its
 * own tile grid (tiles_h - [i == 4 and Ho % 3 != 0]) x (tiles_w - [j == 4 and Wo % 3 != 0]): plane index 4 feeds only a tile's
 * third output row / column, and the products no kept output reads are not computed (81 of 100 per ROI for 5 x 5 outputs).
 * tune_flags bit 17 and bit 7 keep uniform planes. */
MSCNN_API int mscnn_conv2d_plan_plane_columns(const mscnn_conv_plan* plan, int* cols, int n);
/* Roofline accounting: with profiling on, every forward brackets the plan's stages with HIP events on the call's stream;
 * mscnn_conv2d_plan_stage_ms waits for the last forward and returns {input transform, MFMA GEMM kernel(s) incl. the
 * stream-K fix-up, output transform} in milliseconds (direct / head kernels: {0, total, 0}). */
MSCNN_API int mscnn_conv2d_plan_set_profiling(mscnn_conv_plan* plan, int on);
MSCNN_API int mscnn_conv2d_plan_stage_ms(const mscnn_conv_plan* plan, float ms_out[3]);
/* max |x| hand-over between the layers of a chain (split-fp16 plans, MSCNN_CONV_ALGO_WINO_F3_X3).  Such a plan needs an upper
 * bound of max |x| of its input; by default it measures it itself (one streaming pass over x per forward).
 * Both are DEVICE arrays of MSCNN_AMAX_SLOTS uint32 holding float bit patterns; the value they stand for is their maximum
 * (thousands of workgroups publishing into one address would serialise, so each takes one of the slots):
 *   in_bound  (max over the slots >= max |x|; NULL = measure): read by this plan's forward instead;
 *   out_amax  (NULL = off): the plan's forward does atomicMax(bits of a partial max |y|) into the slots -- the caller zeroes
 *             them before the forward.  Only the F(3x3,3x3) forms publish (mscnn_conv2d_plan_publishes_amax() == 1); for other plans a
 *             non-NULL out_amax is MSCNN_ERR_UNSUPPORTED.
 * A max-pooled or ROI-pooled copy of y is bounded by the same value. */
#define MSCNN_AMAX_SLOTS 1024
MSCNN_API int mscnn_conv2d_plan_publishes_amax(const mscnn_conv_plan* plan);
MSCNN_API int mscnn_conv2d_plan_set_amax_io(mscnn_conv_plan* plan, const uint32_t* in_bound, uint32_t* out_amax);
/* Re-shape a plan for a new batch size N (ROI count changes per image, layer.hpp:451-456). */
MSCNN_API int mscnn_conv2d_plan_set_batch(mscnn_conv_plan* plan, int N);
/* Identifies the packed-weight layout the plan currently expects (0: none, the kernel reads the Caffe layout).
 * mscnn_conv2d_plan_set_batch may select a different kernel family for the new batch (e.g. ROI count crossing the
 * Winograd threshold): when this value changes, call mscnn_conv2d_pack_weights again before the next forward. */
MSCNN_API unsigned long long mscnn_conv2d_plan_weight_layout(const mscnn_conv_plan* plan);
/* Alignment: packed 16 (refused); w 4, split-fp16 plans 16 (refused). */
MSCNN_API int mscnn_conv2d_pack_weights(const mscnn_conv_plan* plan, const float* w, float* packed, void* stream);
/* Alignment: packed, workspace 16 (refused); x, y by the plan's kernel -- 4 for the direct kernels, see ALIGNMENT at the top. */
MSCNN_API int mscnn_conv2d_fwd_f32(const mscnn_conv_plan* plan, const float* x, const float* w, const float* packed,
                         const float* bias, float* y, void* workspace, size_t workspace_bytes, void* stream);
/* Convolution (+ the plan's ReLU) with the following PoolingLayer (MAX, kernel 2, stride 2, pad 0, ceil mode:
 * pooling_layer.cu:11-47, pooling_layer.cpp:90-107) fused into the epilogue: y as above AND
 * y_pool[N][Cout][ceil(Ho/2)][ceil(Wo/2)].  Only for plans where mscnn_conv2d_plan_can_pool() is 1 (the trunk
 * kernels); bit-identical to mscnn_conv2d_fwd_f32 followed by mscnn_pool2d_fwd_f32.  y_pool == NULL: plain forward. */
MSCNN_API int mscnn_conv2d_plan_can_pool(const mscnn_conv_plan* plan);
/* Alignment: as mscnn_conv2d_fwd_f32; y_pool 4 (F(4x4,3x3): 8, falls back). */
MSCNN_API int mscnn_conv2d_fwd_pool_f32(const mscnn_conv_plan* plan, const float* x, const float* w, const float* packed,
                              const float* bias, float* y, float* y_pool, void* workspace, size_t workspace_bytes,
                              void* stream);

/* ReLU -- y = max(x, 0) + negative_slope * min(x, 0) as ReLULayer::Forward_cpu writes it (relu_layer.cpp:9-19): NaN stays NaN and
 * signed zeros come out as that layer has them; in place allowed (y == x). */
/* Alignment: 4; falls back from the float4 kernel. */
MSCNN_API int mscnn_relu_fwd_f32(const float* x, float* y, size_t count, float negative_slope, void* stream);

/* Pooling -- PoolingLayer::Forward_gpu (pooling_layer.cu:11-47 MAX, :50-81 AVE; output size
 * pooling_layer.cpp:90-107, ceil mode).  method: 0 MAX, 1 AVE.  The argmax mask the reference
 * also writes is not produced (unused at TEST). */
/* The output shape has one owner.  With either pad non-zero the reference clips the last window of BOTH dimensions
 * (pooling_layer.cpp:94-102), so the two dimensions cannot be sized apart.  Returns MSCNN_ERR_BAD_ARG for what the reference's
 * set-up refuses: pad >= kernel, a last window that still starts in the padding, an empty output. */
MSCNN_API int mscnn_pool_out_dims(int H, int W, int kernel_h, int kernel_w, int pad_h, int pad_w, int stride_h, int stride_w,
                                  int* out_h, int* out_w);
/* One dimension of a pooling with equal pads (pad_h == pad_w); agrees with mscnn_pool_out_dims there. */
MSCNN_API int mscnn_pool_out_dim(int in, int kernel, int pad, int stride);
/* Alignment: 4; the 2x2 / stride 2 fast path (x 16, y 8) falls back. */
MSCNN_API int mscnn_pool2d_fwd_f32(const float* x, float* y, int N, int C, int H, int W, int kernel_h, int kernel_w,
                         int pad_h, int pad_w, int stride_h, int stride_w, int method, void* stream);

/* InnerProduct -- InnerProductLayer::Forward_gpu (inner_product_layer.cu:10-31):
 * y[M,N] = x[M,K] * w[N,K]^T + bias[N]  (transpose_ = false), optional fused ReLU. */
/* Alignment: 4; the MFMA GEMM (x, w 16) falls back to the row-wise / generic kernel. */
MSCNN_API int mscnn_inner_product_fwd_f32(const float* x, const float* w, const float* bias, float* y,
                                int M, int N, int K, int relu, void* stream);
/* dev / test knob of the small-N kernel behind it (cls_pred / bbox_pred): rows of x per workgroup, 2, 4 or 8 (0 = the default: 4 for
 * N <= 5, else 2 -- fewer rows measured faster, profiles/r05_ab_ip_rows.txt).  The per-row arithmetic is the same in every form. */
MSCNN_API void mscnn_debug_inner_product_rows(int rows);

/* The same InnerProduct (fp32, exact MFMA fmaf chains) on the plane-GEMM kernel of the Winograd layers (wgemm.hip: LDS-DMA operand ring,
 * one barrier per K chunk) -- fc6-class shapes: M >= 192 rows, N % 128 == 0, K % 32 == 0 (mscnn_inner_product_wg_supported).  wt = the
 * weights transposed once to [K][N] (mscnn_inner_product_wg_pack, N * K * 4 bytes); x is re-packed into the kernel's A layout every
 * forward inside the workspace; bias and ReLU are applied in the kernel's epilogue.  Results differ from mscnn_inner_product_fwd_f32
 * only in where the K sum is cut (both are k-ordered chains summed in a fixed order: deterministic, within the 1e-4 bar). */
MSCNN_API int mscnn_inner_product_wg_supported(int M, int N, int K);
MSCNN_API size_t mscnn_inner_product_wg_packed_bytes(int N, int K);
MSCNN_API size_t mscnn_inner_product_wg_workspace_bytes(int M, int N, int K);
MSCNN_API int mscnn_inner_product_wg_pack(const float* w, float* wt, int N, int K, void* stream);
/* Alignment: x, wt, workspace 16 (refused); y, bias 4. */
MSCNN_API int mscnn_inner_product_wg_fwd(const float* x, const float* wt, const float* bias, float* y, int M, int N, int K, int relu,
                                         void* workspace, size_t workspace_bytes, void* stream);
/* Health of the plane-GEMM kernel's stream-K hand-off (the Winograd layers and the _wg InnerProduct above).  Where a launch splits
 * its last tiles over workgroups, the workgroup that finishes a tile waits for the others' partial sums; all workgroups of the
 * persistent grid must be co-resident for that (one per CU).  If a contributor never shows up (CU masking, a partition mode the plan
 * was not made for, another stream's kernels holding a CU for > ~0.5 s) the finisher gives up: the tile is stored as NaN (every
 * ReLU behind it keeps a NaN a NaN, as relu_layer.cpp:14-15's std::max does) AND the launch's tag is written to one word of pinned
 * host memory per device.
 *   mscnn_wgemm_handoff_event(): that word for the current device -- 0 = no hand-off has ever timed out; any change since the last
 *     look = at least one launch in between produced a poisoned tile.  Valid once the stream has been synchronised (a plain load).
 *   mscnn_wgemm_force_whole_tiles(1): from now on no launch of this process splits a tile (the last round of tiles is simply not
 *     full: a few % slower on the layers that used the split, never waits for anybody).  The answer to a reported event: force,
 *     then run the frame again -- caffe::Net does exactly that at its synchronisation points (mscnn_net_handoff_state).
 *   mscnn_debug_wgemm_handoff_fault(drop_publish, spin_limit): fault injection for the tests of the above -- contributors never
 *     publish (drop_publish != 0), finishers give up after spin_limit polls (0 = the default 2^22).  Never set in production. */
MSCNN_API unsigned long long mscnn_wgemm_handoff_event(void);
MSCNN_API void mscnn_wgemm_force_whole_tiles(int on);
MSCNN_API int mscnn_wgemm_whole_tiles_forced(void);
MSCNN_API void mscnn_debug_wgemm_handoff_fault(int drop_publish, unsigned spin_limit);
/* Host-side replay of the plane GEMM's schedule for a Winograd plan on the wgemm kernel (tests; runs nothing on a device): every
 * segment the persistent grid's slots are handed, in slot order, as rows {slot, plane, column tile, row tile, k0, k1, part} of 7
 * ints through the kernel's own tile decode (part -1: whole tile); whole_tiles != 0: as after mscnn_wgemm_force_whole_tiles.
 * info[8] = {tiles, MT, KI, G, full_q, planes, BN, ragged}.  Returns the number of segments (rows == NULL: count only), -1 when
 * max_rows is too small or the plan has no such GEMM. */
MSCNN_API long mscnn_debug_wgemm_schedule(const mscnn_conv_plan* plan, int whole_tiles, int* rows, long max_rows, int info[8]);
/* The plan's class (tests; launches nothing, allocates nothing on a device): every discrete decision the plan holds -- kernel family
 * and table entry, operand type, the implicit-GEMM kernel's modes (several M tiles, a partial channel chunk, ROI tiles and a ragged
 * last one, whole tiles / one tile per workgroup / stream-K remainder), the Winograd form (m, nested igemm or wgemm and its tile
 * shape, several row tiles, whole / split remainder / all split, ragged mode, partial edge tiles, small-map transforms), the head
 * kernels' chunk size and schedule, and the
 * can_pool / can_pool_only / publishes_amax / ring / one-launch / Cin = 3 answers -- and nothing that merely scales with the shape.
 * Two plans of one class run the same kernels in the same modes.  *field_names (may be NULL) receives a static comma-separated list
 * naming the ints in order.  Returns the number of fields; fills out[] only when n is at least that. */
MSCNN_API int mscnn_debug_conv_plan_class(const mscnn_conv_plan* plan, int* out, int n, const char** field_names);
/* fp16-operand InnerProduct (the counterpart of MSCNN_CONV_ALGO_F16; no reference counterpart): w16 = the weights converted
 * once to fp16 [N][K] (mscnn_inner_product_pack_f16, N * K * 2 bytes), x rounded to fp16 on its way into LDS, fp32 accumulate.
 * Needs N >= 64 and K % 8 == 0 (mscnn_inner_product_f16_supported); smaller layers stay on the fp32 entry point. */
/* Split-fp16 InnerProduct (fp32-grade: see MSCNN_CONV_ALGO_WINO_F3_X3): w packed once into exactly split fp16 hi + lo units
 * (mscnn_inner_product_x3_pack, mscnn_inner_product_x3_packed_bytes), x split on the device every forward with the scale taken
 * from max |x| -- handed over in in_bound (MSCNN_AMAX_SLOTS uint32, see mscnn_conv2d_plan_set_amax_io) or, when NULL, measured.
 * Three fp16 MFMAs per operand pair, fp32 accumulate, K cut into ranges whose partial sums are added in a fixed order.
 * Needs N >= 128 and K % 32 == 0. */
MSCNN_API int mscnn_inner_product_x3_supported(int N, int K);
MSCNN_API size_t mscnn_inner_product_x3_packed_bytes(int N, int K);
MSCNN_API size_t mscnn_inner_product_x3_workspace_bytes(int M, int N, int K);
MSCNN_API int mscnn_inner_product_x3_pack(const float* w, void* packed, int N, int K, void* stream);
/* Alignment: x, packed, workspace 16 (refused; _pack: w, packed 16); y, bias 4. */
MSCNN_API int mscnn_inner_product_x3_fwd(const float* x, const void* packed, const float* bias, float* y, int M, int N, int K, int relu,
                               const uint32_t* in_bound, void* workspace, size_t workspace_bytes, void* stream);
MSCNN_API int mscnn_inner_product_f16_supported(int N, int K);
MSCNN_API int mscnn_inner_product_pack_f16(const float* w, void* w16, int N, int K, void* stream);
/* Alignment: x, w16 16 (refused); y, bias 4. */
MSCNN_API int mscnn_inner_product_fwd_f16(const float* x, const void* w16, const float* bias, float* y, int M, int N, int K, int relu,
                                          void* stream);

/* Concat along channels -- ConcatLayer::Forward_gpu (concat_layer.cu:9-46).
 * Copies x[N, C, inner] into y[N, C_total, inner] at channel offset c_offset. */
/* Alignment: 4. */
MSCNN_API int mscnn_concat_channels_f32(const float* x, float* y, int N, int C, int inner, int C_total, int c_offset, void* stream);

/* Deconvolution -- DeconvolutionLayer::Forward_gpu (deconv_layer.cu:8-23), depthwise case used by the
 * "-2x" deploy nets (group == Cin == Cout, w[C][1][Kh][Kw], no bias or bias[C]). */
/* Alignment: 4; the 4x4 / stride 2 / pad 1 quad kernel (y 8) falls back. */
MSCNN_API int mscnn_deconv_depthwise_fwd_f32(const float* x, const float* w, const float* bias, float* y,
                                   int N, int C, int H, int W, int Kh, int Kw, int pad_h, int pad_w,
                                   int stride_h, int stride_w, void* stream);

/* Deconvolution, general case (any group / stride / pad; w[Cin][Cout/group][Kh][Kw], base_conv_layer.cpp:135-140 with
 * reverse_dimensions()); routes the depthwise case to the kernel above. */
/* Alignment: 4 (the depthwise case as above). */
MSCNN_API int mscnn_deconv2d_fwd_f32(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int H, int W,
                                     int Cout, int Kh, int Kw, int pad_h, int pad_w, int stride_h, int stride_w, int group,
                                     void* stream);

/* out_dev[0] = max_i |a[i] - ref[i]| / max(floor, |ref[i]|) (+inf if any NaN): the parity metric of the test-suite on the
 * device; used by the host runtime's per-layer numerical calibration (Winograd against the direct sum). */
MSCNN_API int mscnn_max_rel_diff_f32(const float* a, const float* ref, size_t count, float floor, float* out_dev, void* stream);
/* The same metric over `planes` runs of `run` consecutive floats -- plane p of a at a + p * a_stride, of ref at ref + p * ref_stride (a
 * band of rows of an NCHW blob against a band computed elsewhere) -- with floor = max(1, sqrt(sumsq_dev[0] / sumsq_count)) read ON THE
 * DEVICE: the host runtime's numerics watch chains mscnn_sum_squares_f32 -> this call without a host round trip in between. */
MSCNN_API int mscnn_max_rel_diff_strided_f32(const float* a, size_t a_stride, const float* ref, size_t ref_stride, size_t planes, size_t run,
                                             const double* sumsq_dev, double sumsq_count, float* out_dev, void* stream);
/* dst_dev[0 .. n) = values_host[0 .. n), n <= 4, in ONE launch (values travel as kernel arguments): the header words of a detection pack. */
MSCNN_API int mscnn_store_words_i32(int* dst_dev, const int* values_host, int n, void* stream);
/* out_dev[0] = sum_i x[i]^2 in double: the scale (rms) of a blob, the floor of the calibration metric on hot activations. */
MSCNN_API int mscnn_sum_squares_f32(const float* x, size_t count, double* out_dev, void* stream);

/* Softmax over axis 1 of x[outer][C][inner] -- SoftmaxLayer::Forward_gpu (softmax_layer.cu:83-120). */
/* Alignment: 4. */
MSCNN_API int mscnn_softmax_fwd_f32(const float* x, float* y, int outer, int C, int inner, void* stream);

/* ------------------------------------------------------------------------------------------
 * ROIPooling -- ROIPoolingLayer<Dtype>::Forward_gpu (roi_pooling_layer.cu:19-104; CPU twin
 * roi_pooling_layer.cpp:48-139) with the MS-CNN pad_ratio context padding.  rois[R][5] =
 * [batch x1 y1 x2 y2].  Writes out[R][C_total][PH][PW] at channel offset c_offset so that two
 * calls fill the buffer the following Concat layer would produce (C_total == C, c_offset == 0
 * for the stand-alone layer).  A roi's batch index outside [0, N) is NOT checked on the device
 * (the reference CHECKs it on the CPU path only, roi_pooling_layer.cpp:64-65).
 * ------------------------------------------------------------------------------------------ */
/* Alignment: 4. */
MSCNN_API int mscnn_roipool_fwd_f32(const float* feat, const float* rois, float* out, int R, int N, int C, int H, int W,
                          int pooled_h, int pooled_w, float spatial_scale, float pad_ratio,
                          int C_total, int c_offset, void* stream);
/* The same ROIs pooled twice over the same map with two context paddings (roi_pool_org + roi_pool_ctx of the deploy nets,
 * roi_pooling_layer.cu:19-104 twice) into two disjoint channel windows [c_offset_x, c_offset_x + C) of one [R][C_total][ph][pw]
 * output, in one launch. */
/* Alignment: 4. */
MSCNN_API int mscnn_roipool_pair_fwd_f32(const float* feat, const float* rois, float* out, int R, int N, int C, int H, int W,
                                         int pooled_h, int pooled_w, float spatial_scale, float pad_ratio_a, int c_offset_a,
                                         float pad_ratio_b, int c_offset_b, int C_total, void* stream);

/* Chains of same-resolution 3x3 / pad 1 / stride 1 layers on the fp32 F(4x4,3x3) path (conv2_1 -> conv2_2, conv3_1 -> 3_2 -> 3_3,
 * conv4_1 -> 4_2 -> 4_3 of the VGG trunk; the reference runs each as its own cuDNN / im2col call, cudnn_conv_layer.cu:11-46,
 * conv_layer.cu:8-23): the output transform of `plan` writes the input-transform planes of `next` directly -- the activation between the
 * two layers is neither written (unless y != NULL) nor read; 4.5 instead of 6.5 activation-sized HBM passes per pair.  Bit-identical to
 * the two separate mscnn_conv2d_fwd_f32 calls.
 *   _can_chain: 1 when both plans take that path, plan's output is next's input (N, Cout == Cin, H, W) and the map is whole 4x4 tiles
 *     in 1 - 4, 6 or 8 strips of <= 62 tile columns (W <= 1984, W / 4 not in (248, 310] or (372, 434]);
 *   _fwd_chain: x == NULL: the planes of plan's input are already at the start of `workspace` (plan was the `next` of the previous
 *     call on that memory); next == NULL: ordinary output (y required, y_pool optional as in mscnn_conv2d_fwd_pool_f32) -- the tail of
 *     a chain; next != NULL: next's planes go to the start of next_workspace (>= next's mscnn_conv2d_workspace_bytes, disjoint from
 *     `workspace`), y may be NULL, y_pool must be;
 *   _can_pool_only: 1 when a forward with the fused pooling may leave y itself unwritten (y == NULL, y_pool != NULL, here and in
 *     mscnn_conv2d_fwd_pool_f32): the F(4x4,3x3) path and the direct MFMA kernels with the pooling epilogue -- conv1_2, conv2_2,
 *     conv3_3 of the trunk, whose only reader is the pooling layer (283 + 142 + 71 MB per 7s-576 frame not written). */
MSCNN_API int mscnn_conv2d_plan_can_chain(const mscnn_conv_plan* plan, const mscnn_conv_plan* next);
MSCNN_API int mscnn_conv2d_plan_can_pool_only(const mscnn_conv_plan* plan);
/* Alignment: both workspaces 16, y 16 with a next plan (refused); x: falls back. */
MSCNN_API int mscnn_conv2d_fwd_chain_f32(const mscnn_conv_plan* plan, const mscnn_conv_plan* next, const float* x, const float* packed,
                               const float* bias, float* y, float* y_pool, void* workspace, size_t workspace_bytes,
                               void* next_workspace, size_t next_workspace_bytes, void* stream);

/* The detection sub-net's entry fused: ROIPooling x 2 (roi_pooling_layer.cu:19-104, pad_ratio_a -> channels [0, C), pad_ratio_b ->
 * channels [C, 2C) of the concatenated blob, concat_layer.cu:28-46) + the 3x3 convolution that consumes it (roi_c1; conv_layer.cu:8-23)
 * in its Winograd F(3x3,3x3) form: the pooled values go straight into the transform planes of the plane GEMM; the R x 2C x 7 x 7 blob
 * between the layers (140 MB per 7s-576 frame) is neither written nor read.  `plan` = the convolution's plan (N = R ROIs, Cin = 2C,
 * H x W = pooled_h x pooled_w); y = its output, bit-identical to mscnn_roipool_pair_fwd_f32 followed by mscnn_conv2d_fwd_f32.
 *   _can_fuse_roipool: 1 when the plan's kernel family and shape take this path (fp32 F(3x3,3x3), 7 x 7 bins, pad 0, C % 64 == 0);
 *   _roipool_workspace_bytes: workspace of the fused call when it builds its maps itself (the plan's own + mscnn_roipool_maps_bytes);
 *   the pooling reads four "maps" of the feature blob -- a channel-last copy and its sliding maxima over 2 x 2, 4 x 4, 8 x 8 squares
 *   (mscnn_roipool_maps_bytes, mscnn_roipool_maps_build_f32).  They depend on the feature map only: a caller may build them early, on
 *   another stream, while the proposals are still being selected, and hand them in as prepared_maps (then feat may be NULL and the
 *   workspace is the plan's own mscnn_conv2d_workspace_bytes); prepared_maps = NULL builds them inside the call. */
MSCNN_API int mscnn_conv2d_plan_can_fuse_roipool(const mscnn_conv_plan* plan, int C, int pooled_h, int pooled_w);
MSCNN_API size_t mscnn_conv2d_roipool_workspace_bytes(const mscnn_conv_plan* plan, int N, int C, int H, int W);
MSCNN_API size_t mscnn_roipool_maps_bytes(int N, int C, int H, int W);
/* Alignment: maps 16 (refused); feat 4. */
MSCNN_API int mscnn_roipool_maps_build_f32(const float* feat, float* maps, int N, int C, int H, int W, void* stream);
/* Alignment: prepared_maps, workspace, packed_w 16 (refused); feat, rois, y 4 (y: scalar staging where it is not 16-byte aligned). */
MSCNN_API int mscnn_conv2d_fwd_roipool_pair_f32(const mscnn_conv_plan* plan, const float* feat, const float* prepared_maps, int N, int C,
                                                int H, int W, const float* rois, float spatial_scale, float pad_ratio_a,
                                                float pad_ratio_b, const float* packed_w, const float* bias, float* y, void* workspace,
                                                size_t workspace_bytes, void* stream);

/* ROIAlign -- ROIAlignLayer<Dtype>::Forward_gpu (roi_align_layer.cu:21-112): out[R][C][pooled_h+1][pooled_w+1] bilinear
 * samples on the grid of the (context-padded) roi; the WiderFace cascade deploy follows it with a 2x2 stride-1 AVE Pooling. */
/* Alignment: 4. */
MSCNN_API int mscnn_roialign_fwd_f32(const float* feat, const float* rois, float* out, int R, int N, int C, int H, int W,
                                     int pooled_h, int pooled_w, float spatial_scale, float pad_ratio, void* stream);
/* ROIAlign (roi_align_layer.cu:21-98) + the 2x2 / stride 1 / pad 0 AVE Pooling that follows it in the deploy
 * (pooling_layer.cu:50-81), written into channels [c_offset, c_offset + C) of out[R][C_total][pooled_h][pooled_w].  The grid of samples
 * stays in LDS.  Every value is bit-identical to mscnn_roialign_fwd_f32 -> mscnn_pool2d_fwd_f32 (AVE, 2, 2, pad 0, stride 1) ->
 * mscnn_concat_channels_f32: the sample is the same device function, the average is the pooling kernel's sum order and division.
 * Refused before any launch (MSCNN_ERR_BAD_ARG, the text names the argument): a null pointer, a non-positive shape, a channel window
 * outside [0, C_total), and a grid of more than 256 points: (pooled_h + 1) * (pooled_w + 1) <= 256, i.e. up to 15 x 15 bins.
 * R == 0 returns MSCNN_OK and touches nothing.  A roi's batch index outside [0, N) is NOT checked, as in ROIPooling and ROIAlign. */
/* Alignment: 4. */
MSCNN_API int mscnn_roialign_ave_fwd_f32(const float* feat, const float* rois, float* out, int R, int N, int C, int H, int W,
                                         int pooled_h, int pooled_w, float spatial_scale, float pad_ratio,
                                         int C_total, int c_offset, void* stream);
/* The same ROIs sampled with two context paddings into two disjoint channel windows of one output: the five layers
 * roi_grid_org / roi_pool_org / roi_grid_ctx / roi_pool_ctx / roi_pool (Concat) of the WiderFace cascade in one launch.
 * Refusals as above, plus windows that overlap. */
/* Alignment: 4. */
MSCNN_API int mscnn_roialign_ave_pair_fwd_f32(const float* feat, const float* rois, float* out, int R, int N, int C, int H, int W,
                                              int pooled_h, int pooled_w, float spatial_scale, float pad_ratio_a, int c_offset_a,
                                              float pad_ratio_b, int c_offset_b, int C_total, void* stream);

/* Eltwise -- EltwiseLayer<Dtype>::Forward_gpu (eltwise_layer.cu): op 0 PROD, 1 SUM (coeffs_host[num_bottoms], NULL = all 1),
 * 2 MAX.  bottoms_host: host array of num_bottoms (2..8) device pointers of `count` floats each. */
/* Alignment: 4. */
MSCNN_API int mscnn_eltwise_fwd_f32(const float* const* bottoms_host, int num_bottoms, const float* coeffs_host, float* y,
                                    size_t count, int op, void* stream);

/* ------------------------------------------------------------------------------------------
 * BoxOutput -- BoxOutputLayer<Dtype>::Forward_cpu (box_output_layer.cpp:66-234; the reference has
 * no GPU version, box_output_layer.hpp:39-40): per-anchor decode + filter, descending sort on
 * (score, candidate index), top max_nms_num, greedy NMS (nmsMax :38-63, BoxIOU
 * math_functions.cpp:12-35), emit rois [b x1 y1 x2 y2] and proposals+score [b x1 y1 x2 y2 s].
 * ------------------------------------------------------------------------------------------ */
#define MSCNN_BOXOUT_MAX_HEADS 16
typedef struct {
  int num_heads;                              /* number of bottoms */
  int num;                                    /* batch size (images) */
  int channels;                               /* cls_num + 4 */
  int head_h[MSCNN_BOXOUT_MAX_HEADS], head_w[MSCNN_BOXOUT_MAX_HEADS];
  float field_w[MSCNN_BOXOUT_MAX_HEADS], field_h[MSCNN_BOXOUT_MAX_HEADS], downsample_rate[MSCNN_BOXOUT_MAX_HEADS];
  float fg_thr, iou_thr;
  int nms_mode;                               /* 0 "IOU", 1 "IOMU", 2 "IOFU" */
  float field_whr, field_xyr;
  int max_nms_num, max_post_nms_num;
  float min_size;
  int do_bbox_norm;                           /* bbox_reg_param present with 4 means and 4 stds */
  float bbox_mean[4], bbox_std[4];
} mscnn_boxoutput_desc;

MSCNN_API size_t mscnn_boxoutput_workspace_bytes(const mscnn_boxoutput_desc* desc);
/* Row capacity needed for rois_out / props_out / anchor_ids_out. */
MSCNN_API int mscnn_boxoutput_max_rows(const mscnn_boxoutput_desc* desc);
/*
 * heads_host: host array of num_heads DEVICE pointers.  rois_out[cap][5], props_out[cap][6]
 * (NULL allowed), anchor_ids_out[cap] (NULL allowed; global anchor id = head offset + h*w index of
 * each emitted row, -1 for the dummy row), count_out_dev: device int[2] = {R, num_real}
 * (R includes the dummy row [0 1 1 10 10] emitted when nothing survives, :195-199).
 * Asynchronous on `stream`; the caller copies count_out_dev back when it needs R on the host.
 */
/* Alignment: workspace 16 (refused); everything else 4. */
MSCNN_API int mscnn_boxoutput_fwd_f32(const mscnn_boxoutput_desc* desc, const float* const* heads_host,
                            float* rois_out, float* props_out, int* anchor_ids_out, int cap,
                            int* count_out_dev, void* workspace, size_t workspace_bytes, void* stream);
/*
 * The same layer with every image of the batch side by side.  Arguments, contract and refusals are those of
 * mscnn_boxoutput_fwd_f32, and every output word is bit-identical to it: rois, props, anchor ids, both count words, the rows
 * grouped by image in image order, the dummy row only when no image of the batch keeps a box.  desc->num images run in groups of
 * up to 32: five launches per group (decode + filter with the image on a grid axis, one select-and-sort workgroup per image, the
 * NMS bit matrix with the image on blockIdx.z, one greedy-scan workgroup per image, then one small launch in which each image's
 * workgroup sums the row counts of the images in front of it and writes its rows) where the per-image op takes four launches per
 * image.  No workgroup waits for another; exactly one thread of the call's last launch stores count_out_dev[0..1], once, and
 * nothing else stores there (it may be host-coherent memory that the host reads behind an event on `stream`; the words say how
 * many rows the batch has, not that every image's rows have landed -- only the end of that launch does).  One image, and a
 * descriptor on the large path (max_nms_num 0, or above 4032 with that many anchors), are served by mscnn_boxoutput_fwd_f32
 * itself.  The workspace holds that op's workspace plus min(num, 32) per-image slices (1.9 MB each at 45,630 anchors and
 * max_nms_num 2000); it is 0 with mscnn_last_error set for a bad descriptor.
 */
MSCNN_API size_t mscnn_boxoutput_batch_workspace_bytes(const mscnn_boxoutput_desc* desc);
/* Alignment: workspace 16 (refused); everything else 4. */
MSCNN_API int mscnn_boxoutput_batch_fwd_f32(const mscnn_boxoutput_desc* desc, const float* const* heads_host,
                            float* rois_out, float* props_out, int* anchor_ids_out, int cap,
                            int* count_out_dev, void* workspace, size_t workspace_bytes, void* stream);

/* Greedy NMS on already score-sorted boxes [n][4] = x y w h (nmsMax, greedy = true):
 * keep_out[n] bytes 0/1.  Exposed for the index-exactness parity tests. */
MSCNN_API size_t mscnn_nms_workspace_bytes(int n);
/* Alignment: boxes_xywh, workspace 16 (refused). */
MSCNN_API int mscnn_nms_greedy_f32(const float* boxes_xywh, int n, float iou_thr, int nms_mode, unsigned char* keep_out,
                         void* workspace, size_t workspace_bytes, void* stream);

/* DecodeBBox (TEST phase) -- DecodeBBoxLayer<Dtype>::Forward_cpu (decode_bbox_layer.cpp:54-123,
 * DecodeBBoxesWithPrior math_functions.cpp:46-75); bbox[R][8] (columns 4..7 used), prior[R][5],
 * mean/std host arrays of 4.  A std that is not > 0 (zero, negative, NaN) is refused with the value named, as the reference's
 * set-up does (decode_bbox_layer.cpp:30). */
/* Alignment: 4. */
MSCNN_API int mscnn_decodebbox_fwd_f32(const float* bbox, const float* prior, float* out, int R, int bbox_dim,
                             const float* mean_host, const float* std_host, void* stream);

/* ------------------------------------------------------------------------------------------
 * Final detection stage -- the MATLAB post-processing the reference runs on the net outputs
 * (examples/kitti_car/run_mscnn_detection.m:75-120, utils/bbNms.m:112-126): proposal filter,
 * bbox de-normalisation + transform, softmax prob of class cls_id (1-based), rescale to the
 * original image, clip, greedy NMS (stable sort, union, double precision).
 * dets_out[cap][5] doubles [x y w h prob], ids_out[cap] input row of each detection,
 * count_out_dev: device int[1] = D.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  int ncls, cls_id;
  float bbox_mean[4], bbox_std[4];
  float proposal_thr;
  double ratio_h, ratio_w, org_h, org_w, nms_overlap;
} mscnn_detections_desc;
MSCNN_API size_t mscnn_detections_workspace_bytes(int R);

/* bbNms's user knobs (utils/bbNms.m:49-56, `pNms` at the top of every reference driver), one setting per call.  The calls without
 * this struct, a NULL pointer and the all-default struct are the same thing: nmsMax(greedy = 1, ovrDnm = union), thr = -inf, and
 * their results are byte-identical.
 *   type     'maxg' (greedy: a suppressed box suppresses nothing) or 'max' (box j goes when ANY higher-scored box overlaps it,
 *            suppressed or not: bbNms.m:117 with greedy = 0 -- on the device a column-OR of the overlap bit matrix instead of the
 *            serial scan).  Refused, naming the value: 'ms' (mean shift needs nonMaxSuprList, which the reference does not ship),
 *            'cover' (its scores come from a BLAS mat-vec, N * bbs(:,5), whose summation order can not be pinned, so no bit-exact
 *            restatement exists) and 'none' (read the ROI rows instead).
 *   ovr_dnm  'union': o / (as_i + as_j - o); 'min': o / min(as_i, as_j) (bbNms.m:121).  Doubles, the same operation order, strict
 *            o > nms_overlap (nms_overlap stays in mscnn_detections_desc).
 *   thr      rows with !(prob > thr) are dropped before the NMS (bbNms.m:85, strict).  Encoding: the value itself, a double;
 *            the default is -HUGE_VAL (-inf, bbNms's own default), any other non-NaN value is a threshold (+inf drops every row).
 *   det_thr  plain stage only (examples/widerface/run_mscnn_detection.m:139-143): when > 0, rows with !(prob >= det_thr) are
 *            dropped before the NMS.  0 = off.  The cascade calls keep their own det_thr argument and refuse a non-zero one here.
 * Not covered: maxn (split-and-recurse, a heuristic that changes results: only its default inf -- mscnn_nms_params_from_names
 * refuses a finite one), radii ('ms' only), resize and separate (no reference driver sets them).
 * More than 4032 rows in one list (the tiled path) run with the default setting only; anything else is refused there. */
enum { MSCNN_NMS_TYPE_MAXG = 0, MSCNN_NMS_TYPE_MAX = 1, MSCNN_NMS_TYPE_MS = 2, MSCNN_NMS_TYPE_COVER = 3, MSCNN_NMS_TYPE_NONE = 4 };
enum { MSCNN_NMS_OVR_UNION = 0, MSCNN_NMS_OVR_MIN = 1 };
#ifndef MSCNN_NMS_PARAMS_DEFINED
#define MSCNN_NMS_PARAMS_DEFINED
typedef struct {
  int type;          /* 0 = 'maxg', 1 = 'max' */
  int ovr_dnm;       /* 0 = 'union', 1 = 'min' */
  double thr;        /* -HUGE_VAL = bbNms's default -inf */
  float det_thr;     /* 0 = off; plain stage only */
} mscnn_nms_params;
#endif
/* Validates *nms (NULL: the defaults) and writes the setting the kernels will run with to *out, every byte of it (padding zero):
 * everything a nms pointer contributes to a launch.  Fails, naming the value, on a refused or out-of-range field. */
MSCNN_API int mscnn_nms_params_resolve(const mscnn_nms_params* nms, mscnn_nms_params* out);
/* The same from bbNms's own spelling: type 'maxg' / 'max', ovr_dnm 'union' / 'min' (NULL: the default), thr, maxn (must be
 * HUGE_VAL = inf), det_thr. */
MSCNN_API int mscnn_nms_params_from_names(const char* type, const char* ovr_dnm, double thr, double maxn, float det_thr,
                                          mscnn_nms_params* out);
/* Alignment (all mscnn_detections_* calls): workspace, pack_dev 16, dets_out 8 (refused); the blobs, ids_out, count_out_dev 4. */
MSCNN_API int mscnn_detections_fwd(const mscnn_detections_desc* desc, const float* bbox_pred, const float* cls_pred,
                         const float* props, int R, double* dets_out, int* ids_out, int* count_out_dev,
                         void* workspace, size_t workspace_bytes, void* stream);

MSCNN_API int mscnn_detections_nms_fwd(const mscnn_detections_desc* desc, const mscnn_nms_params* nms, const float* bbox_pred,
                                       const float* cls_pred, const float* props, int R, double* dets_out, int* ids_out,
                                       int* count_out_dev, void* workspace, size_t workspace_bytes, void* stream);

/* Final stage of the cascade drivers (examples/kitti_car/run_cascademscnn.m:84-117): `boxes` = the decoded box blob of a
 * cascade stage [R][5] = [img x1 y1 x2 y2] (DecodeBBox output), `cls_prob` = that stage's in-net probabilities [R][ncls]
 * (Softmax / Eltwise blob), `props` = its proposal blob [R][5].  Rescale, clip, w = x2 - x1 + 1, drop rows whose proposal
 * has zero width or height, optional det_thr (> 0), then the same NMS.  desc: ncls, cls_id, ratio_*, org_*, nms_overlap. */
MSCNN_API int mscnn_detections_cascade_fwd(const mscnn_detections_desc* desc, float det_thr, const float* boxes,
                                 const float* cls_prob, const float* props, int R, double* dets_out, int* ids_out,
                                 int* count_out_dev, void* workspace, size_t workspace_bytes, void* stream);
MSCNN_API int mscnn_detections_cascade_nms_fwd(const mscnn_detections_desc* desc, float det_thr, const mscnn_nms_params* nms,
                                               const float* boxes, const float* cls_prob, const float* props, int R, double* dets_out,
                                               int* ids_out, int* count_out_dev, void* workspace, size_t workspace_bytes, void* stream);

/* The same stage for EVERY (image, class) segment of a batched forward in one pass (three launches per 32 segments, no host
 * read).  props / bbox_pred / cls_pred hold the ROIs of num_images images, grouped by image with the image index in column 0 of
 * props (BoxOutput's layout); each segment finds its own rows on the device.  desc[num_images * num_classes], indexed
 * [image * num_classes + class]: per-segment cls_id, ratios, original size, thresholds (ncls equal in all).  max_rows_per_image:
 * a host-known bound on any image's rows (BoxOutput's max_nms_num, or R_all), at most 4032 -- above that run mscnn_detections_fwd
 * per segment.  Every segment is bit-identical to mscnn_detections_fwd on its row range, ids included.
 * pack_dev (mscnn_detections_multi_pack_bytes(S, cap) bytes, S = num_images * num_classes, cap >= num_classes * R_all):
 *   [int32 S, R_all, cap, 0][S x int32 {count, rows, row0, 0}][cap x 5 doubles x y w h prob][cap x int32 id]
 * segment s = (image i, class c) owns pack rows [num_classes * row0 + c * rows, + rows), ids relative to its row0; count -1: the
 * image had more rows than max_rows_per_image (nothing was run for it).  Every word of the header and table is written by the
 * kernels; rows of a slot past its count are left as they were.  The layout below is the one definition every writer and
 * reader of the pack uses (K = slots per image: num_classes here, num_outputs * num_classes in the cascade call). */
enum { MSCNN_MULTI_PACK_WORDS = 4 };      /* int32 words of the header and of every table entry: entry s at word 4 * (1 + s) */
typedef struct { size_t dets, ids, total; } mscnn_multi_pack_layout;      /* byte offsets of dets (= the table's bytes) and ids, pack bytes */
static inline mscnn_multi_pack_layout mscnn_multi_pack_layout_of(int num_segments, int cap) {
  const size_t S = (size_t)(num_segments > 0 ? num_segments : 0), rows = (size_t)(cap > 0 ? cap : 1);
  mscnn_multi_pack_layout L;
  L.dets = sizeof(int32_t) * MSCNN_MULTI_PACK_WORDS * (1 + S);
  L.ids = L.dets + rows * 5 * sizeof(double);
  L.total = (L.ids + rows * sizeof(int32_t) + 15) / 16 * 16;
  return L;
}
#ifdef __HIPCC__      /* the kernels that write the pack place their slots with it too */
__host__ __device__
#endif
static inline size_t mscnn_multi_pack_slot(int K, int row0, int k, int rows) {      /* first pack row of slot k of an image */
  return (size_t)K * row0 + (size_t)k * rows;
}
MSCNN_API size_t mscnn_detections_multi_pack_bytes(int num_segments, int cap);
MSCNN_API size_t mscnn_detections_multi_workspace_bytes(int num_segments, int max_rows_per_image);   /* 0: over 4032 rows */
MSCNN_API int mscnn_detections_multi_fwd(const mscnn_detections_desc* desc, int num_images, int num_classes, const float* bbox_pred,
                                         const float* cls_pred, const float* props, int R_all, int max_rows_per_image, void* pack_dev,
                                         int cap, void* workspace, size_t workspace_bytes, void* stream);
/* ... with bbNms's knobs (one setting for all segments); mscnn_detections_multi_fwd is this call with nms = NULL. */
MSCNN_API int mscnn_detections_multi_nms_fwd(const mscnn_detections_desc* desc, const mscnn_nms_params* nms, int num_images,
                                             int num_classes, const float* bbox_pred, const float* cls_pred, const float* props,
                                             int R_all, int max_rows_per_image, void* pack_dev, int cap, void* workspace,
                                             size_t workspace_bytes, void* stream);

/* The same one-pass stage for the cascade drivers (mscnn_detections_cascade_fwd per segment): several sources instead of one.
 * outputs[num_outputs], 1 <= num_outputs <= 4: each cascade output's own blob triple (boxes [R_all][5], cls_prob [R_all][ncls],
 * props [R_all][5]; R_all common to all); each segment finds its rows in ITS output's props.  desc[num_images * num_outputs *
 * num_classes], indexed [(image * num_outputs + output) * num_classes + class]: cls_id (1 .. that output's ncls), ratio_*, org_*,
 * nms_overlap; the other fields (ncls included: it comes from outputs[]) are not read.  det_thr: one value per call.  Every segment
 * is bit-identical to mscnn_detections_cascade_fwd on its row range of its output's blobs, ids included.  pack_dev: the multi pack
 * with K = num_outputs * num_classes slots per image, cap >= K * R_all; segment (i, o, c) owns slot k = o * num_classes + c. */
typedef struct {
  const float* boxes;
  const float* cls_prob;
  const float* props;
  int ncls;
} mscnn_cascade_output;
MSCNN_API size_t mscnn_detections_cascade_multi_workspace_bytes(int num_segments, int max_rows_per_image);   /* 0: over 4032 rows */
MSCNN_API int mscnn_detections_cascade_multi_fwd(const mscnn_detections_desc* desc, float det_thr, int num_images, int num_outputs,
                                                 int num_classes, const mscnn_cascade_output* outputs, int R_all,
                                                 int max_rows_per_image, void* pack_dev, int cap, void* workspace,
                                                 size_t workspace_bytes, void* stream);
/* ... with bbNms's knobs; mscnn_detections_cascade_multi_fwd is this call with nms = NULL. */
MSCNN_API int mscnn_detections_cascade_multi_nms_fwd(const mscnn_detections_desc* desc, float det_thr, const mscnn_nms_params* nms,
                                                     int num_images, int num_outputs, int num_classes,
                                                     const mscnn_cascade_output* outputs, int R_all, int max_rows_per_image,
                                                     void* pack_dev, int cap, void* workspace, size_t workspace_bytes, void* stream);

/* Several forwards of an image, ONE NMS: input sizes (multi-scale testing), a mirrored frame, tiles of a frame too large for one
 * forward.  The rows that survive the final stage's row transform stay on the device, per segment, in original-image coordinates
 * (the candidates); the sort, bit matrix and scan of the calls above then run once over each list (the merge).
 * A segment is (image, class) for the plain stage and (image, cascade output, class) for the cascade stage, S of them, indexed as
 * the desc of the multi calls above.  cand: one device buffer of mscnn_detections_candidates_bytes(S, cand_cap) bytes (0: refused
 * arguments) -- per segment two int32 {rows that wanted in, overflow flag} and cand_cap slots of box (4 doubles), prob (float) and
 * tag (int32).  Layout, each array at the next multiple of 256 bytes, list s in slots [s * cand_cap, + cand_cap) of each:
 *   [S x int32 {wanted, overflow}][S cand_cap x 4 doubles x y w h][S cand_cap x float prob][S cand_cap x int32 tag]
 * mscnn_detections_candidates_reset zeroes every count and flag (the slots are left as they are).
 *
 * mscnn_detections_candidates_add / _cascade_add take the arguments of mscnn_detections_multi_nms_fwd /
 * mscnn_detections_cascade_multi_nms_fwd for ONE forward: each segment finds its image's rows in props, every row goes through the
 * very row transform and filters of those calls (proposal filter, thr / det_thr of nms included), and the forward's view is applied
 * in double to the box [x y w h] that came out:
 *     x' = flip_x ? (double)org_w - (x + w) : x        org_w = the desc's, as the float the row was clipped against
 *     x' = x' + off_x,  y' = y + off_y                  w, h and prob are untouched
 * view[num_images], one per image; NULL = the identity (the box bit for bit).  The desc's org_h / org_w and ratios describe the
 * VIEW -- the tile or the whole frame at this forward's input size --, the offsets place it in the original image.  The cascade
 * rows keep their w = x2 - x1 + 1 convention; the same formula applies to them.  Survivors are appended behind the segment's
 * count in row order (one workgroup per segment, steps of 256 rows, ballot / popcount prefix, no atomics), so a list's order is
 * (order of the add calls, row) whatever the timing.  tag = (pass << 24) | row, row = the row of that forward's ROI blobs
 * (absolute in the batch: the convention of the multi calls' ids + row0).  A list that would pass cand_cap stores nothing past the
 * cap, sets its overflow flag and keeps counting the rows that wanted in: never a silent truncation.  One launch per 32 segments.
 *
 * mscnn_detections_merge_fwd: the NMS over each list.  Sort key: larger prob first, then the earlier candidate -- a tie between
 * two passes goes to the pass added first, inside a pass to the lower row.  nms_overlap[S]: a HOST array, one per segment.  Of nms,
 * type and ovr_dnm are read here (thr and det_thr were applied by the add calls).  cand_cap <= 4032: all segments in one pass, three
 * launches per 32 segments, no host read.  cand_cap > 4032: list after list on the tiled kernels, each list's length read from its
 * device count; the default type / ovr_dnm only, anything else is refused naming the limit.
 * pack_dev: the multi pack, mscnn_multi_pack_layout_of(S, S * cand_cap):
 *   [int32 S, cand_cap, S * cand_cap, 0][S x int32 {count, candidates, s * cand_cap, 0}][S cand_cap x 5 doubles][S cand_cap x int32 tag]
 * segment s owns pack rows [s * cand_cap, + cand_cap) and fills the first count; count -1: the list overflowed (candidates = the
 * rows that wanted in, nothing was run).  The kernels write every header and table word; rows of a slot past its count are left as
 * they were.  workspace: mscnn_detections_merge_workspace_bytes(S, cand_cap) bytes (0: refused arguments).
 * Refused before any launch, naming the value: null pointers, S < 1, cand_cap < 1 (or S * cand_cap past 2^31 - 1), pass outside
 * [0, 127], R_all < 1 or >= 2^24, a NaN or non-positive ratio, a NaN overlap, a non-finite offset, a flip_x that is neither 0 nor 1,
 * a workspace that is too small, cand / workspace / pack_dev not 16-byte aligned, a non-zero nms det_thr in the cascade add.
 * No pin on the reference: its scripts run one forward per image.  The check is a numpy restatement (tests/merge_witness.py), and
 * one add + merge is bit-identical to mscnn_detections_multi_nms_fwd / mscnn_detections_cascade_multi_nms_fwd on the same blobs. */
#ifndef MSCNN_DETECTIONS_VIEW_DEFINED
#define MSCNN_DETECTIONS_VIEW_DEFINED
typedef struct { double off_x, off_y; int flip_x; } mscnn_detections_view;
#endif
MSCNN_API size_t mscnn_detections_candidates_bytes(int num_segments, int cand_cap);
MSCNN_API int mscnn_detections_candidates_reset(void* cand, int num_segments, int cand_cap, void* stream);
MSCNN_API int mscnn_detections_candidates_add(const mscnn_detections_desc* desc, const mscnn_detections_view* view,
                                              const mscnn_nms_params* nms, int pass, int num_images, int num_classes,
                                              const float* bbox_pred, const float* cls_pred, const float* props, int R_all, void* cand,
                                              int cand_cap, void* stream);
MSCNN_API int mscnn_detections_candidates_cascade_add(const mscnn_detections_desc* desc, const mscnn_detections_view* view, float det_thr,
                                                      const mscnn_nms_params* nms, int pass, int num_images, int num_outputs,
                                                      int num_classes, const mscnn_cascade_output* outputs, int R_all, void* cand,
                                                      int cand_cap, void* stream);
/* The images of ONE batched forward into the lists of the FRAMES they are views of: a frame and its mirror, or the tiles of a frame,
 * run as the batch they naturally are.  desc[num_images * K] and view[num_images] describe the images of THIS forward exactly as in
 * _add / _cascade_add (K = num_classes, resp. num_outputs x num_classes); list_of[num_images] is a HOST array: the rows of image b
 * go to the lists of frame list_of[b], cand has S = num_lists * K lists (list = list_of[b] * K + slot).  Every row goes through the
 * one row transform and the view arithmetic of _add (flip_x against the desc's org_w, then + off_x, + off_y, in double); the tag is
 * (pass << 24) | row with row absolute in the batch.
 * ORDER of a list: (add call, image index ascending, row) -- never a matter of timing.  One workgroup owns a list and walks its
 * images in turn (the table of a launch holds 32 (image, slot) pairs, grouped by list): no atomics on global memory, no workgroup
 * waits on another, nothing spins.  With more pairs than one launch holds, later launches continue the lists in stream order, the
 * count read from the device.  Counts, the overflow flag and "nothing stored past the cap" are those of _add: a list keeps counting
 * the rows that wanted in.  list_of = {0, 1, ..., N - 1} with num_lists == num_images leaves the whole cand buffer byte-identical
 * to _add.
 * Refused before any launch, naming the value: everything _add / _cascade_add refuse, a null list_of, num_lists < 1, an entry of
 * list_of outside [0, num_lists).  mscnn_detections_merge_fwd then runs as it is (its limit above 4032 slots included).
 * No pin on the reference (its scripts have neither views nor a merge): the check is tests/merge_witness.py with the passes listed
 * in (add, image) order. */
MSCNN_API int mscnn_detections_candidates_add_views(const mscnn_detections_desc* desc, const mscnn_detections_view* view, const int* list_of,
                                                    const mscnn_nms_params* nms, int pass, int num_images, int num_lists, int num_classes,
                                                    const float* bbox_pred, const float* cls_pred, const float* props, int R_all,
                                                    void* cand, int cand_cap, void* stream);
MSCNN_API int mscnn_detections_candidates_cascade_add_views(const mscnn_detections_desc* desc, const mscnn_detections_view* view,
                                                            const int* list_of, float det_thr, const mscnn_nms_params* nms, int pass,
                                                            int num_images, int num_lists, int num_outputs, int num_classes,
                                                            const mscnn_cascade_output* outputs, int R_all, void* cand, int cand_cap,
                                                            void* stream);
MSCNN_API size_t mscnn_detections_merge_workspace_bytes(int num_segments, int cand_cap);
MSCNN_API int mscnn_detections_merge_fwd(const double* nms_overlap, const mscnn_nms_params* nms, int num_segments, void* cand,
                                         int cand_cap, void* pack_dev, void* workspace, size_t workspace_bytes, void* stream);

/* Box voting, the other half of the multi-scale / flip / tiled testing recipe: the merge above SELECTS one box per cluster, this op
 * then REFINES each kept box from everything the forwards said about it.  Call it after mscnn_detections_merge_fwd with the same
 * cand, cand_cap and pack_dev (either merge path: the op reads the candidate buffer and the pack only, and needs no workspace).
 * Per segment s with table count D >= 0, for every kept row k < D with box A = [x y w h] as it stands in the pack: candidate
 * j = 0 .. min(wanted, cand_cap) - 1 of the list, box B and prob p_j, VOTES when o / u >= thr, o and u in double exactly as the NMS
 * computes them for ovr_dnm = union --
 *     iw = fmin(A.x + A.w, B.x + B.w) - fmax(A.x, B.x)   (iw <= 0: no vote);   ih likewise;   o = iw * ih;   u = A.w * A.h + B.w * B.h - o
 * -- a NaN ratio does not vote; the union form always, whatever ovr_dnm the NMS ran with.  With weights (double)p_j the row's box
 * becomes [sum p x / sum p, sum p y / sum p, sum p w / sum p, sum p h / sum p], written IN PLACE over the four box doubles of pack
 * row s * cand_cap + k.  The vote runs on x y w h as they are: the cascade rows keep their w = x2 - x1 + 1 convention.
 * A kept row with fewer than two voters stays bit for bit as it was, and so does one whose sum p is not > 0.  Nothing else is
 * written: not the prob column, the tags, the header, the table, rows past a count, nor any slot of a segment with count -1.
 * A row reads the candidates, never other pack rows, so in place is safe; calling the op TWICE votes again around the moved boxes:
 * it is not idempotent.
 * SUMMATION ORDER, part of the contract (fixed by the slot index alone, never by grid size, scheduling or timing): 64 partial sums
 * per quantity; partial l adds the voters among slots l, l + 64, l + 128, ... in ascending order, each term p * v rounded, then
 * added (no fma), starting from +0.0; the partials v[0 .. 63] are combined by an xor butterfly, for m = 32, 16, 8, 4, 2, 1:
 * v[l] = v[l] + v[l ^ m] for all l at once; the result is v[0] (every v[l] holds the same bits); then the four divisions.
 * One launch for all segments, a fixed grid, no host read, no atomics.
 * Refused before the launch, naming the value: a null pointer, S < 1, cand_cap < 1 (or S * cand_cap past 2^31 - 1), a thr that is
 * NaN or outside (0, 1), cand or pack_dev not 16-byte aligned.
 * No pin on the reference: its scripts neither merge nor vote.  The check is tests/vote_witness.py: a numpy restatement with this
 * summation order, compared bit for bit, and an exact-rational mean over the same voters. */
typedef struct { double thr; } mscnn_vote_params;     /* 0 < thr < 1 */
MSCNN_API int mscnn_detections_merge_vote_fwd(const mscnn_vote_params* vote, int num_segments, const void* cand, int cand_cap,
                                              void* pack_dev, void* stream);

/* Soft-NMS over the merged candidates (Bodla et al., 2017), beside mscnn_detections_merge_fwd: where the hard NMS deletes every
 * candidate that overlaps a kept box, this op DECAYS its score -- the form the multi-scale / flip / tiled recipe is most often run
 * with in crowded scenes, where two true objects overlap by more than the NMS threshold and N forwards make every cluster N times
 * denser.  It reads the candidate buffer exactly as mscnn_detections_merge_fwd does and writes the same multi pack,
 * mscnn_multi_pack_layout_of(S, S * cand_cap): header {S, cand_cap, S * cand_cap, 0}, table entry {count, wanted, s * cand_cap, 0}
 * (count -1: the list overflowed, nothing else of it is written), rows [x y w h score] + tag in PICK order -- so
 * mscnn_detections_merge_vote_fwd and every reader of the merge's pack work on it unchanged.  The kernels write every header and
 * table word; rows of a slot past its count are left as they were; cand is read only.
 * Per segment s, with n = min(wanted, cand_cap) candidates in slot order (wanted < 0: n = 0), s_j = (double)prob_j, all live, D = 0:
 *   1. stop when nothing is live, or when max_out > 0 && D == max_out;
 *   2. m = the live candidate with the largest s; among equal s the lowest slot index wins -- the merge's own tie rule: the pass
 *      added first, then the lower row.  A NaN s ranks below every number (and with the NaNs and -inf, again the lowest slot);
 *   3. stop when !(s_m >= score_thr);
 *   4. pack row s * cand_cap + D = box m bit for bit, s_m, tag m; m is dead; D = D + 1;
 *   5. for every live j, with A = box m and B = box j, in double, the vote's overlap statements, the union form always:
 *          iw = fmin(A.x + A.w, B.x + B.w) - fmax(A.x, B.x)   (iw <= 0: no decay);   ih likewise;
 *          o = iw * ih;   u = A.w * A.h + B.w * B.h - o;   r = o / u                  (a NaN r: no decay)
 *          MSCNN_SOFT_NMS_LINEAR:    if (r > nms_overlap[s]) s_j = s_j * (1.0 - r)
 *          MSCNN_SOFT_NMS_GAUSSIAN:  s_j = s_j * exp(-(r * r) / sigma)                (nms_overlap is not read)
 *      every operation rounded, no fma; back to 1.
 * The argmax is a maximum under a TOTAL order (score, then the lower slot), so the result depends on no reduction shape, grid size,
 * scheduling or timing; no atomics.  The linear method is IEEE operations only and is bit-exact against tests/soft_witness.py; the
 * gaussian one calls the device library's exp (picks and counts exact while no two scores lie within a few ulps of each other).
 * ANY cand_cap is served: one workgroup of 1024 threads owns a list; a list whose count is <= 4096 lives in registers, a longer one
 * keeps its scores and live flags in the workspace and reads the boxes from cand -- the same arithmetic per candidate, the same bits.
 * workspace: mscnn_detections_merge_soft_workspace_bytes(S, cand_cap) bytes (0: refused arguments).  nms_overlap[S]: a HOST array.
 * Refused before any launch, naming the value: null pointers, S < 1, cand_cap < 1 (or S * cand_cap past 2^31 - 1), a method outside
 * {1, 2}, gaussian with a sigma that is not finite or not > 0, a score_thr that is NaN, infinite or < 0, max_out < 0, a NaN overlap
 * with linear, cand / workspace / pack_dev not 16-byte aligned, a workspace that is too small (MSCNN_ERR_WORKSPACE).
 * No pin on the reference: its scripts neither merge nor decay a score.  The check is tests/soft_witness.py: a float64 numpy
 * restatement of the five steps (linear: bit for bit) and the linear method in exact rationals. */
enum { MSCNN_SOFT_NMS_LINEAR = 1, MSCNN_SOFT_NMS_GAUSSIAN = 2 };
typedef struct { int method; double sigma; double score_thr; int max_out; } mscnn_soft_nms_params;
MSCNN_API size_t mscnn_detections_merge_soft_workspace_bytes(int num_segments, int cand_cap);
MSCNN_API int mscnn_detections_merge_soft_fwd(const double* nms_overlap, const mscnn_soft_nms_params* soft, int num_segments, void* cand,
                                              int cand_cap, void* pack_dev, void* workspace, size_t workspace_bytes, void* stream);

/* Matrix NMS over the merged candidates (Wang et al., "SOLOv2", NeurIPS 2020, Algorithm 1), beside mscnn_detections_merge_fwd and
 * mscnn_detections_merge_soft_fwd: a score decay like Soft-NMS's, but with NO pick loop -- every candidate's decay is a min over
 * the candidates ranked above it, compensated by their column maxima of the same IoU matrix: two parallel passes over the upper
 * triangle instead of n serial picks.  It does NOT return Soft-NMS's scores: a decay here is the worst single pair, compensated,
 * not a product over picks.  The op reads the candidate buffer exactly as the merge does and only reads it, and writes the same
 * multi pack, mscnn_multi_pack_layout_of(S, S * cand_cap): header {S, cand_cap, S * cand_cap, 0}, table entry {count, wanted,
 * s * cand_cap, 0} (count -1: the list overflowed, nothing else of it is written), rows [x y w h score'] + tag; rows past a count
 * are left as they were; the kernels write every header and table word; mscnn_detections_merge_vote_fwd and every reader of the
 * pack work on the result unchanged.  Per segment (-ffp-contract=off holds for the library: no fma):
 *   1. n = min(wanted, cand_cap), and n = 0 when wanted < 0.  The candidates are put in the merge's own order: larger prob first,
 *      then the earlier slot (det_key(prob, slot)).  Call the sorted positions 0 .. n-1, with s_j = (double)prob_j.
 *   2. For i < j, with A = box i and B = box j, the overlap uses the vote's and Soft-NMS's statements, always in union form:
 *          iw = fmin(A.x + A.w, B.x + B.w) - fmax(A.x, B.x);   ih likewise;
 *          o = iw * ih;   u = A.w * A.h + B.w * B.h - o;   r_ij = o / u;
 *      r_ij = 0.0 where iw <= 0, ih <= 0 or the ratio is a NaN.
 *   3. Compensation is the column maximum: c_i = max over k < i of r_ki, and c_0 = 0.0.
 *   4. Decay of j >= 1, MSCNN_MATRIX_NMS_LINEAR: d_j = min over i < j of (1.0 - r_ij) / (1.0 - c_i), starting from 1.0.  A term
 *      whose 1.0 - c_i is not > 0 is skipped (such an i is an exact duplicate of a higher-ranked box, and that box already
 *      contributes the same term; the skip also keeps 0/0 out).  A NaN term is skipped, which is fmin's rule.  score'_j = s_j * d_j.
 *   5. Decay of j >= 1, MSCNN_MATRIX_NMS_GAUSSIAN: g_j = max over i < j of (r_ij * r_ij - c_i * c_i) / sigma, starting from 0.0; a
 *      NaN term is skipped.  score'_j = s_j * exp(-g_j): ONE exp per candidate, not one per pair (min_i exp(a_i) = exp(min_i a_i)).
 *      sigma divides, as in mscnn_soft_nms_params, so 0.5 means the same thing in both ops.
 *   6. score'_0 = s_0.
 *   7. The candidates with score' >= score_thr are kept (a NaN fails the test).  They come out in descending score' order, equal
 *      scores ordered by the lower sorted position.  The first max_out are taken when max_out > 0.  count is their number.  Pack
 *      row s * cand_cap + k holds box k of that order bit for bit, then score', then the tag.
 * The order in 7 is a total order and the reductions in 3 to 5 are exact (min and max of non-NaN doubles), so no reduction shape,
 * grid size, scheduling or timing decides a bit.  No atomics on global memory, nothing spins, no workgroup waits on another.  The
 * linear method is IEEE operations only and is bit-exact against tests/matrix_witness.py; the gaussian one calls the device
 * library's exp once per candidate.
 * Lists of at most 4032 slots are sorted by the merge's one-pass sort, all segments side by side, 32 per launch; longer ones go list
 * after list through the tiled path's key kernel, sort and gather (cand_cap up to 2^30, the sort's largest power of two).  Then, per
 * 32 segments: compensation pass, decay pass (r_ij recomputed: no n x n matrix of doubles is stored), one score launch, a rank pass
 * (the output position of j = the number of kept candidates before it in the order of 7) and the emit.
 * workspace: mscnn_detections_merge_matrix_workspace_bytes(S, cand_cap) bytes, linear in cand_cap (0: refused arguments).
 * Refused before any launch, naming the value: null pointers, S < 1, cand_cap < 1 (or S * cand_cap past 2^31 - 1, or cand_cap past
 * 2^30), a method outside {1, 2}, gaussian with a sigma that is not finite or not > 0, a score_thr that is NaN, infinite or < 0,
 * max_out < 0, cand / workspace / pack_dev not 16-byte aligned, a workspace that is too small (MSCNN_ERR_WORKSPACE).
 * No pin on the reference: its scripts neither merge nor decay a score.  The check is tests/matrix_witness.py: a float64 numpy
 * restatement of the seven steps (linear: bit for bit), a plain triple loop, and the linear method in exact rationals.  The accuracy
 * of Matrix NMS against Soft-NMS was not evaluated: there are no labels here. */
enum { MSCNN_MATRIX_NMS_LINEAR = 1, MSCNN_MATRIX_NMS_GAUSSIAN = 2 };
typedef struct { int method; double sigma; double score_thr; int max_out; } mscnn_matrix_nms_params;
MSCNN_API size_t mscnn_detections_merge_matrix_workspace_bytes(int num_segments, int cand_cap);   /* 0: refused arguments */
MSCNN_API int mscnn_detections_merge_matrix_fwd(const mscnn_matrix_nms_params* mx, int num_segments, void* cand, int cand_cap,
                                                void* pack_dev, void* workspace, size_t workspace_bytes, void* stream);

/* Weighted boxes fusion over the merged candidates (WBF; Solovyev, Wang, Gabruseva, "Weighted boxes fusion: Ensembling boxes from
 * different object detection models", 2019 / Image and Vision Computing 2021), beside mscnn_detections_merge_fwd, _soft_fwd and
 * _matrix_fwd.  Those three SELECT or RE-SCORE single candidates; this op builds CLUSTERS while it walks the list in score order:
 * a cluster's box is the score-weighted mean of all its members, that mean is what the next candidate is matched against, and a
 * cluster's confidence is scaled by how many of the forwards agreed on it, min(members, T) / T.  Box voting is not a substitute: it
 * refines boxes the hard NMS already picked, against the picked box, and never touches a score.  The op reads the candidate buffer
 * exactly as the merge does and only reads it, and writes the same multi pack, mscnn_multi_pack_layout_of(S, S * cand_cap): header
 * {S, cand_cap, S * cand_cap, 0}, table entry {count, wanted, s * cand_cap, 0} (count -1: the list overflowed, nothing else of it is
 * written), rows [x y w h conf] + tag; rows past a count are left as they were; the kernels write every header and table word, so
 * every reader of the merge's pack works on the result unchanged.  Per segment s, everything in double (-ffp-contract=off holds for
 * the library: every operation rounded, no fma):
 *   1. n = min(wanted, cand_cap), and n = 0 when wanted < 0.  The candidates are walked in the merge's own order, det_key(prob, slot):
 *      larger prob first, then the lower slot; a NaN prob ranks below every number.  s_i = (double)prob_i.
 *   2. Candidate i ENTERS while s_i >= skip_thr && s_i > 0; the walk ends at the first candidate that fails this test (the order
 *      makes that the same as filtering).
 *   3. Its box B is matched against the fused boxes F_c of the clusters that exist, c = 0 .. C-1 in creation order.  The overlap uses
 *      the vote's, Soft-NMS's and Matrix NMS's statements with A = F_c, the union form always:
 *          iw = fmin(A.x + A.w, B.x + B.w) - fmax(A.x, B.x)   (iw <= 0: no match);   ih likewise;
 *          o = iw * ih;   u = A.w * A.h + B.w * B.h - o;   r = o / u                  (a NaN r: no match)
 *      The candidate joins the cluster with the largest r among those with r > thr; among equal r the lowest c.  nms_overlap and
 *      the sticky nms type / ovr_dnm are not read.
 *   4. No such cluster: a new cluster C with members = 1, sw = s_i, sx = s_i * B.x (sy, sW, sH likewise), F_C = B BIT FOR BIT -- a
 *      cluster of one gives back its candidate's box unchanged --, first = i: its tag and its s_i are the cluster's own.
 *   5. Otherwise sw = sw + s_i; sx = sx + s_i * B.x -- the product rounded, then the sum -- and the same for y, w, h; members += 1;
 *      F_c = [sx / sw, sy / sw, sW / sw, sH / sw].  The sums run in walk order: the summation order is part of the contract and is
 *      fixed by the list alone.  The cascade rows keep their w = x2 - x1 + 1 convention (a mean of x y w h is the mean of the corners).
 *   6. After the walk, per cluster: conf = sw / (double)members (MSCNN_WBF_CONF_AVG) or conf = s_first (MSCNN_WBF_CONF_MAX: the walk
 *      is in descending score, so the first member is the largest); then conf = conf * (double)min(members, expected[s]) /
 *      (double)expected[s].
 *   7. The clusters come out in descending conf, equal conf ordered by the lower cluster index; with max_out > 0 only the first
 *      max_out.  count is their number.  Pack row s * cand_cap + k holds the fused box, conf and the tag of the cluster's first member;
 *      with a non-NULL members_dev, members_dev[s * cand_cap + k] holds its member count.  Entries past a count and entries of an
 *      overflowed list are not written.
 * The match in 3 and the order in 7 are maxima under total orders, so no reduction shape, grid size, scheduling or timing decides a
 * bit; IEEE operations only: bit-exact against tests/wbf_witness.py.  No atomics on global memory, nothing spins, no workgroup
 * waits on another.
 * ANY cand_cap up to 2^30 (the sort's largest power of two) is served.  Lists of at most 4032 slots are sorted by the merge's
 * one-pass sort, 32 segments per launch; longer ones go list after list through the tiled path's key kernel, sort and gather.  One
 * workgroup of 1024 threads then owns a list and walks it, a step = one overlap per existing cluster spread over the lanes and one
 * argmax over (r, lower c), reduced over the waves that own a cluster.  A list whose count is <= 4096 keeps the fused boxes of its
 * clusters in registers; a longer one reads them from the workspace -- the same arithmetic, the same bits.  The five running sums of
 * a cluster are touched by one lane per step and live in the workspace.
 * expected[S]: a HOST array, each >= 1 (the number of forwards that looked at the list).  workspace:
 * mscnn_detections_merge_wbf_workspace_bytes(S, cand_cap) bytes, linear in cand_cap (0: refused arguments).
 * Refused before any launch, naming the value: a null wbf / expected / cand / pack_dev / workspace (members_dev may be NULL), S < 1,
 * cand_cap < 1 (or S * cand_cap past 2^31 - 1, or cand_cap past 2^30), a thr that is NaN or outside (0, 1), a skip_thr that is NaN,
 * infinite or < 0, a conf_type outside {1, 2}, max_out < 0, an expected[s] < 1, cand / workspace / pack_dev not 16-byte aligned,
 * members_dev not 4-byte aligned, a workspace that is too small (MSCNN_ERR_WORKSPACE).
 * No pin on the reference: its scripts run one forward per image and neither merge nor fuse.  The check is tests/wbf_witness.py: a
 * float64 numpy restatement of the seven steps (bit for bit) and the same walk in exact rationals.  The accuracy of WBF against the
 * hard merge, Soft-NMS and Matrix NMS was NOT evaluated: there are no labels here. */
enum { MSCNN_WBF_CONF_AVG = 1, MSCNN_WBF_CONF_MAX = 2 };
typedef struct { double thr; double skip_thr; int conf_type; int max_out; } mscnn_wbf_params;
MSCNN_API size_t mscnn_detections_merge_wbf_workspace_bytes(int num_segments, int cand_cap);      /* 0: refused arguments */
MSCNN_API int mscnn_detections_merge_wbf_fwd(const mscnn_wbf_params* wbf, const int* expected /* HOST, [S], each >= 1 */,
                                             int num_segments, void* cand, int cand_cap, void* pack_dev,
                                             int* members_dev /* may be NULL; [S * cand_cap] int32 */, void* workspace,
                                             size_t workspace_bytes, void* stream);

/* Seq-NMS over the candidate lists of a clip's frames (Han, Khorrami, Paine et al., "Seq-NMS for Video Object Detection", 2016),
 * beside mscnn_detections_merge_fwd, _soft_fwd, _matrix_fwd and _wbf_fwd.  Those combine the views of ONE frame; this op lets the
 * frames of a clip inform one another: it links the boxes of neighbouring frames by overlap, repeatedly takes the chain of boxes
 * with the largest score sum, gives every box of the chain the chain's score, and suppresses what the chain's boxes overlap in their
 * own frames.  Every detection also gets a sequence id (a tubelet).  S = num_frames * num_slots segments; segment s = t * K + k is the
 * list of frame t, slot k -- the layout the candidate adds produce (list = frame x K + slot; K = classes, or outputs x classes for the
 * cascade).  Chain k is the segments k, K + k, ..., (T - 1) K + k; chains never interact.  The op reads the candidate buffer exactly
 * as the merge does and only reads it, and writes the same multi pack, mscnn_multi_pack_layout_of(S, S * cand_cap): header
 * {S, cand_cap, S * cand_cap, 0}, table entry {count, wanted, s * cand_cap, 0}, rows [x y w h score'] + tag; every header and table
 * word is written, rows past a count are left as they were.  Per chain, everything in double (-ffp-contract=off holds for the
 * library: every operation rounded, no fma, IEEE operations only):
 *   1. Entry.  Per segment n = min(wanted, cand_cap), and n = 0 when wanted < 0.  An overflowed list gets table count -1, nothing
 *      else of it is written, and it takes part as an EMPTY frame.  The list is put in the merge's own order, det_key(prob, slot):
 *      larger prob first, then the lower slot; a NaN ranks below every number.  s_i = (double)prob_i.  The candidates that ENTER are
 *      the leading ones with s_i >= score_thr (a NaN fails), at most top_k of them: boxes 0 .. m_t - 1 of frame t.
 *   2. Links.  For t >= 1, box (t-1, i) and box (t, j) are linked iff the overlap with A = box (t-1, i), B = box (t, j) is > link_thr,
 *      in the vote's, Soft-NMS's, Matrix NMS's and WBF's statements, the union form:
 *          iw = fmin(A.x + A.w, B.x + B.w) - fmax(A.x, B.x)   (iw <= 0: no link);   ih likewise;
 *          o = iw * ih;   u = A.w * A.h + B.w * B.h - o;   r = o / u                  (a NaN r: no link)
 *   3. Start.  All entered boxes are live, q = 0.  Steps 4 - 10 repeat while the chain has a live box.
 *   4. DP, frames ascending.  For a live (t, j) let P be the live boxes i of frame t - 1 linked to j.  t = 0 or P empty: V = s_tj,
 *      len = 1, prev = -1.  Otherwise p = the member of P with the largest V(t-1, .), among equal V the lowest i; V(t, j) =
 *      V(t-1, p) + s_tj -- one rounded add, so a path's sum runs in frame order from its first box --, len = len_p + 1, prev = p.
 *      (Scores are >= score_thr >= 0: a path is always extended when it can be.)
 *   5. The end of the best path: the live box with the largest V; among equal V the lower t, then the lower j.  The path is the end
 *      box followed back through prev.
 *   6. score' = V_end / (double)len_end (MSCNN_SEQ_NMS_AVG) or the largest s on the path (MSCNN_SEQ_NMS_MAX).
 *   7. Every box of the path is OUT: its own box bit for bit, score', its own tag, sequence id q.  It is dead from then on.
 *   8. Suppression.  For every path box (t, j*), every live j of frame t whose overlap with A = box j*, B = box j is
 *      > nms_overlap[t * K + k] dies and is never output.  The union form always: the sticky nms type / ovr_dnm are not read, thr /
 *      det_thr were applied by the adds.
 *   9. q = q + 1.
 *  10. Every iteration kills at least the end box: at most sum m_t iterations, a bound the kernel's loop carries.  Nothing spins, no
 *      workgroup waits on another, no atomics on global memory.
 *  11. The rows of a segment: its output boxes in descending score', equal scores ordered by the lower sorted position; with
 *      max_out > 0 only the first max_out.  count is their number.  With a non-NULL seq_dev, seq_dev[s * cand_cap + row] holds the
 *      sequence id.  Entries past a count and entries of an overflowed list are not written.  max_out cuts the OUTPUT only: it does
 *      not shorten the loop, every sequence is still formed and suppresses.
 * Steps 4, 5 and 11 take maxima under total orders and every sum has its order fixed by the path, so no reduction shape, grid size,
 * scheduling or timing decides a bit: bit-exact against tests/seq_witness.py.
 * Lists of at most 4032 slots are sorted by the merge's one-pass sort, 32 segments per launch; longer ones go list after list through
 * the tiled path's key kernel, sort and gather.  One parallel launch builds the link bits of every (chain, frame pair): row j of frame
 * t holds top_k bits over frame t - 1.  One workgroup of 1024 threads then owns a chain, a thread = a box of the frame at hand (hence
 * top_k <= 1024); the live masks of all frames and the previous frame's V / len sit in LDS (59 KB), prev in the workspace; an
 * iteration costs num_frames + 3 workgroup barriers and a serial walk back through prev.  The DP restarts at frame 0 in every
 * iteration; the overlaps of step 8 are recomputed, not stored.  A last launch, a workgroup per segment, ranks and writes the rows.
 * nms_overlap[S]: a HOST array.  workspace: mscnn_detections_merge_seq_workspace_bytes(num_frames, num_slots, cand_cap, top_k)
 * bytes = the sort's need + S * top_k * (8 * ceil(top_k / 64) + 60) and a few rounded-up tables (0: refused arguments).
 * Refused before any launch, naming the value: a null nms_overlap / sq / cand / pack_dev / workspace (seq_dev may be NULL),
 * num_frames outside [1, 256], num_slots < 1, cand_cap < 1 (or S * cand_cap past 2^31 - 1, or cand_cap past 2^30), top_k outside
 * [1, 1024], a link_thr that is NaN or outside (0, 1), a score_thr that is NaN, infinite or < 0, a rescore outside {1, 2},
 * max_out < 0, a NaN nms_overlap[s], cand / workspace / pack_dev not 16-byte aligned, seq_dev not 4-byte aligned, a workspace that
 * is too small (MSCNN_ERR_WORKSPACE).
 * No pin on the reference: its scripts run one forward per image and look at no other frame.  The check is tests/seq_witness.py: a
 * float64 numpy restatement of the eleven steps (bit for bit), the same loop in exact rationals and a brute force over every linked
 * path of tiny chains.  The accuracy of Seq-NMS was NOT evaluated: there are no labels here. */
enum { MSCNN_SEQ_NMS_AVG = 1, MSCNN_SEQ_NMS_MAX = 2 };
typedef struct { double link_thr; double score_thr; int top_k; int rescore; int max_out; } mscnn_seq_nms_params;
MSCNN_API size_t mscnn_detections_merge_seq_workspace_bytes(int num_frames, int num_slots, int cand_cap, int top_k); /* 0: refused */
MSCNN_API int mscnn_detections_merge_seq_fwd(const double* nms_overlap /* HOST, [S] */, const mscnn_seq_nms_params* sq,
                                             int num_frames, int num_slots, void* cand, int cand_cap, void* pack_dev,
                                             int* seq_dev /* may be NULL; [S * cand_cap] int32 */, void* workspace,
                                             size_t workspace_bytes, void* stream);

/* A streaming multi-object tracker behind the final stage: BYTE association on the device (Zhang et al., "ByteTrack: Multi-Object
 * Tracking by Associating Every Detection Box", 2022).  A small table of tracks per slot (class, or output x class) lives in device
 * memory from call to call; every new frame's detections are associated with the tracks in two passes -- the high-score detections
 * first, then the low-score detections against the tracks still unmatched -- and every detection row gets a persistent track id.
 * Two things THIS op does in its own way, each with the paper's way on request beside it: its motion is a constant-velocity
 * prediction of the box centre (the paper's Kalman filter: mscnn_tracks_update_kalman_fwd below), and its matching is greedy by
 * descending overlap under a total order (the optimal assignment that SORT, DeepSORT and ByteTrack solve:
 * mscnn_tracks_update_assign_fwd below).  Both make the result independent of reduction shape and scheduling: bit-exact against
 * tests/track_witness.py.
 * pack_dev: a multi pack as mscnn_detections_multi_fwd, the merge ops and Seq-NMS write it, mscnn_multi_pack_layout_of(S, cap) with
 * S = num_frames * num_slots; segment s = t * K + k is frame t, slot k.  The op only reads it.  The segment's rows [x y w h score]
 * start at its ROW OFFSET: table word 2 as the merge ops write it (s * cand_cap); in the pack of a batched forward, where the K
 * slots of an image carry the same {rows, row0} -- told apart on the device by the first two entries of the frame having the same
 * word 2, which no merged pack has --, mscnn_multi_pack_slot(K, row0, k, rows).  The frames of a call are consecutive frames of the
 * stream in ascending t; the calls follow each other in stream order.  Slots never interact.
 * state: per slot a header of MSCNN_TRACKS_HEADER_WORDS int32 {n, next_id, frame, dropped, skipped, steps, 0, 0} (steps: word
 * MSCNN_TRACKS_STEPS, written 0 by this op, see mscnn_tracks_update_assign_fwd), behind it max_tracks
 * records (mscnn_track_record); mscnn_tracks_state_layout_of names the offsets.  mscnn_tracks_state_reset sets n = 0, next_id = 1,
 * frame = 0, dropped = skipped = 0.  state_in == state_out (in place) and two distinct buffers both work; records at index >= n of
 * state_out are left as they were.  track_ids_dev: cap int32, one per pack row.
 * Per slot and frame, all in double, every operation rounded (no fma):
 *   1. frame += 1.
 *   2. Entry.  count = the segment's table count.  count < 0 (an overflowed list) is an EMPTY frame: m = 0 and its track ids are not
 *      written (so is a segment whose rows [offset, offset + count) do not lie inside the pack's cap rows).  Otherwise m = min(count,
 *      1024), skipped += count - m.  Detection j = pack row j of the segment, s_j its score.  H = {j: s_j >= high_thr}, L = {j:
 *      low_thr <= s_j < high_thr}; a NaN score is in neither.
 *   3. Predict.  MSCNN_TRACK_MOTION_LINEAR: box.x += vel.x, box.y += vel.y for every track.  MSCNN_TRACK_MOTION_NONE: nothing.
 *   4. Pass 1.  Every track i with every j in H: r(i, j) = the overlap with A = the track's box, B = the detection, in the vote's,
 *      Soft-NMS's, Matrix NMS's, WBF's and Seq-NMS's statements, the union form:
 *          iw = fmin(A.x + A.w, B.x + B.w) - fmax(A.x, B.x)   (iw <= 0: no pair);   ih likewise;
 *          o = iw * ih;   u = A.w * A.h + B.w * B.h - o;   r = o / u                  (a NaN r: no pair)
 *      A pair is eligible iff r > match_thr.  The eligible pairs are walked in the total order larger r, then the lower i, then the
 *      lower j; a pair whose track and detection are both still free is matched.
 *   5. Pass 2 (BYTE).  The tracks unmatched after pass 1 with misses == 0 and confirmed != 0 (seen in the previous frame) with every
 *      j in L, eligible iff r > match_thr_low, the same walk.  low_thr == high_thr: L is empty, a plain greedy IoU tracker.
 *   6. Matched (i, j).  g = misses + 1.  With MOTION_LINEAR dx = ((B.x + B.w / 2) - (obs.x + obs.w / 2)) / (double)g, dy likewise;
 *      hits == 1: vel = (dx, dy); otherwise vel.x = vel.x + vel_gain * (dx - vel.x), vel.y likewise.  Then box = obs = B bit for bit,
 *      score = s_j, hits += 1, misses = 0, confirmed |= (hits >= min_hits).
 *   7. Unmatched track.  misses += 1; it keeps its predicted box, obs unchanged; it dies when confirmed == 0 or misses > max_age.
 *   8. Births.  Every unmatched j in H with s_j >= new_thr, in ascending j: box = obs = B, vel = 0, score = s_j, hits = 1, misses = 0,
 *      confirmed = (min_hits <= 1).
 *   9. Compaction.  The survivors in their old order, then the births in ascending j; the first max_tracks are kept.  Births that do
 *      not fit are dropped (dropped += their number, no id); the kept births take id = next_id++ in their order.  Table order is
 *      age order, which is what the tie-break of step 4 reads.
 *  10. track_ids_dev[row offset + j], j < count: the id of the track detection j was matched to or started, if that track is
 *      confirmed after this frame, else 0.  Entries past count are not written.
 * The walk of steps 4 and 5 runs as rounds of "match every mutually-best pair": the order on pairs is total, so a pair that is the
 * best remaining pair of both its track and its detection is picked by the walk before any other pair that uses either, and the
 * rounds give the same matching (tests/track_witness.py does both).  The loop carries its own bound, min(tracks, detections)
 * rounds.  One launch per call, one workgroup of 1024 threads per slot looping over the frames, a thread = a track and a detection
 * (hence the two 1024 bounds); one 32 KB box buffer in LDS holds the tracks' and the detections' boxes in turn (58 KB in all); the
 * table is loaded once per call and stored once.  Nothing spins, no workgroup waits on another, no atomics.
 * Refused before any launch, naming the value: a null params / pack_dev / state_in / state_out / track_ids_dev, num_frames < 1,
 * num_slots < 1, cap < 1 (or S * cap past 2^31 - 1), max_tracks outside [1, 1024], a NaN high_thr / low_thr / new_thr, a match_thr
 * or match_thr_low that is NaN or outside [0, 1), low_thr > high_thr, new_thr < high_thr, vel_gain outside (0, 1], a motion outside
 * {1, 2}, max_age < 0, min_hits < 1, pack_dev / state_in / state_out not 16-byte aligned, track_ids_dev not 4-byte aligned, state_in
 * and state_out overlapping without being equal.
 * No pin on the reference: its scripts run one forward per image and look at no other frame.  The check is tests/track_witness.py: a
 * float64 numpy restatement of the ten steps (bit for bit), with the walk done literally and by mutually-best rounds.  The accuracy
 * of the tracker was NOT evaluated: there are no labels here. */
enum { MSCNN_TRACK_MOTION_NONE = 1, MSCNN_TRACK_MOTION_LINEAR = 2 };
#ifndef MSCNN_TRACK_PARAMS_DEFINED
#define MSCNN_TRACK_PARAMS_DEFINED
typedef struct { double high_thr, low_thr, new_thr, match_thr, match_thr_low, vel_gain;
                 int motion, max_age, min_hits; } mscnn_track_params;
#endif
enum { MSCNN_TRACKS_N = 0, MSCNN_TRACKS_NEXT_ID = 1, MSCNN_TRACKS_FRAME = 2, MSCNN_TRACKS_DROPPED = 3, MSCNN_TRACKS_SKIPPED = 4,
       MSCNN_TRACKS_STEPS = 5 /* mscnn_tracks_update_assign_fwd's optimal form; 0 otherwise */, MSCNN_TRACKS_HEADER_WORDS = 8 };      /* int32 words of a slot's header */
typedef struct { double box[4], obs[4], vel[2], score; int32_t id, hits, misses, confirmed; } mscnn_track_record;      /* 104 bytes */
typedef struct { size_t records, record, slot, total; } mscnn_tracks_state_layout;   /* byte offset of a slot's records, bytes of a record, of a slot, of the state */
static inline mscnn_tracks_state_layout mscnn_tracks_state_layout_of(int num_slots, int max_tracks) {
  const size_t K = (size_t)(num_slots > 0 ? num_slots : 0), M = (size_t)(max_tracks > 0 ? max_tracks : 0);
  mscnn_tracks_state_layout L;
  L.records = sizeof(int32_t) * MSCNN_TRACKS_HEADER_WORDS;
  L.record = sizeof(mscnn_track_record);
  L.slot = L.records + M * L.record;
  L.total = (K * L.slot + 15) / 16 * 16;
  return L;
}
MSCNN_API size_t mscnn_tracks_state_bytes(int num_slots, int max_tracks);      /* 0: refused arguments */
MSCNN_API int mscnn_tracks_state_reset(void* state, int num_slots, int max_tracks, void* stream);
MSCNN_API int mscnn_tracks_update_fwd(const mscnn_track_params* params, int num_frames, int num_slots, const void* pack_dev, int cap,
                                      const void* state_in, void* state_out, int max_tracks,
                                      int* track_ids_dev /* [cap] int32, one per pack row */, void* stream);

/* The tracker for a batch of STREAMS (cameras): a batch in live video is one frame from each of several cameras, not several frames
 * of one, and every camera needs a table of its own.  Frame t of the pack belongs to stream stream_of[t], inside [0, num_streams);
 * the frames of stream s in this call are the t with stream_of[t] == s in ascending t, consecutive frames of that stream.  A stream
 * may have no frame in a call.  state: mscnn_tracks_state_layout_of(num_streams * num_slots, max_tracks); the table of (stream s,
 * slot k) is slot s * num_slots + k of it.  Per (stream, slot) the ten steps above run unchanged over that stream's frames: header,
 * records and the frame counter are the stream's own, ids are unique within a (stream, slot) and start at 1 in each.  A stream with
 * no frame in the call: its block of state_out equals its block of state_in in the header and the first n records (with two distinct
 * buffers too), its frame counter does not move, no track of it ages.  track_ids_dev as above: every pack row < count of every frame
 * of the call is written, nothing else.
 * One launch: a workgroup of 1024 threads per (slot, stream), grid (num_slots, num_streams); every workgroup walks t = 0 ..
 * num_frames - 1 and skips the frames of the other streams -- on a kernel argument and its own block index, a value every thread of
 * the workgroup reads alike, so every barrier is still reached by all.  No atomics, nothing spins, no workgroup waits on another; the
 * same 58 KB of LDS.  stream_of is a HOST array, read before the call returns; it travels BY VALUE in the kernel's arguments (256
 * entries of 16 bits), so there is no allocation, no copy and no synchronisation inside the op -- hence, when num_streams > 1,
 * num_frames <= 256 and num_streams <= 256.  mscnn_tracks_update_fwd is this op with num_streams = 1, on the same kernel.
 * Refused before any launch, naming the value: everything mscnn_tracks_update_fwd refuses (with S * cap and num_streams * num_slots
 * held below 2^31), a null stream_of, num_streams outside [1, 256], num_frames > 256 with more than one stream, an entry of stream_of
 * outside [0, num_streams) (naming t and the entry).
 * mscnn_tracks_state_reset_slots resets the tables [first_slot, first_slot + count) of a state of num_slots_total tables -- one
 * camera starts again, the others keep their tracks -- and touches no other byte.  (mscnn_tracks_state_reset can not be pointed at a
 * sub-block: a table is 32 + 104 * max_tracks bytes, 8-byte but not always 16-byte aligned.)  It refuses a null or unaligned state
 * and a range outside [0, num_slots_total]; count 0 does nothing.
 * No pin on the reference here either; the check is the same witness run per stream on that stream's frames
 * (tests/track_streams_witness.py).  The accuracy was NOT evaluated. */
MSCNN_API int mscnn_tracks_update_streams_fwd(const mscnn_track_params* params, int num_frames, int num_slots, int num_streams,
                                              const int* stream_of /* HOST, [num_frames] */, const void* pack_dev, int cap,
                                              const void* state_in, void* state_out, int max_tracks, int* track_ids_dev, void* stream);
MSCNN_API int mscnn_tracks_state_reset_slots(void* state, int num_slots_total, int max_tracks, int first_slot, int count, void* stream);

/* The tracker with the paper's motion model: a constant-velocity Kalman filter per track on (cx, cy, a = w / h, h), as SORT, DeepSORT
 * and ByteTrack run it, in the place of steps 3 and 6's linear prediction.  A second setting beside mscnn_track_params, a side table
 * beside the track state, an entry point of its own: mscnn_track_params, mscnn_track_record and the two ops above do not change, and
 * MSCNN_TRACK_MOTION_NONE / _LINEAR stay what they are (on a noise-free approaching box the linear rule overlaps better than the
 * filter: the filter is an option, not a replacement).  The matching of THIS op is the greedy walk; mscnn_tracks_update_assign_fwd
 * below runs the filter under either matching.
 * ONE argument: the op would have 17, so it takes a pointer to a call struct that carries them all, the stream among them (`size`
 * must be sizeof(mscnn_tracks_kalman_call)).  The stream contract binds it as every op: it waits for nothing and runs in the order of
 * call->stream.  call->track, call->filter, call->stream_of are HOST and read before the call returns.
 * With a diagonal start, diagonal noise and a position-only measurement the eight-state filter decouples exactly into four two-state
 * filters (component c: position x[c], velocity v[c]), so a record holds per component the position's variance p, the covariance q and
 * the velocity's variance r: 12 covariance numbers, no matrix is inverted.  mscnn_track_kalman_record: x = (cx, cy, a, h), v their
 * velocities, (p, q, r) as said.  filter_in / filter_out: num_streams * num_slots * max_tracks records, the record of track i of
 * table (s, k) at index (s * num_slots + k) * max_tracks + i -- beside record i of that table in the state.  There is no header and
 * no reset op: a filter record is initialised at its track's birth, and a table with n = 0 has none.
 * The ten steps of mscnn_tracks_update_streams_fwd run unchanged except as follows; track->motion must be MSCNN_TRACK_MOTION_NONE,
 * vel_gain is not read.  With sp, sv, sa, sav, sam = std_position, std_velocity, std_aspect, std_aspect_velocity, std_aspect_measure,
 * all in double, one rounding per operation, in exactly this order:
 *   3'. Predict, every track.  freeze_lost_height != 0 and misses > 0: v[3] = 0.  h = x[3]; e = sp * h; g = sv * h;
 *       sigp = {e, e, sa, e}, sigv = {g, g, sav, g}.  Per component:
 *           x = x + v;  t0 = p + q;  t1 = q + r;  p = (t0 + t1) + sigp * sigp;  q = t1;  r = r + sigv * sigv
 *       Then w = x[2] * x[3]; box = {x[0] - w / 2, x[1] - x[3] / 2, w, x[3]}; vel = {v[0], v[1]}.
 *   6'. Matched with detection B.  z = {B.x + B.w / 2, B.y + B.h / 2, B.w / B.h, B.h}; h = x[3] (the predicted one); e = sp * h;
 *       sigm = {e, e, sam, e}.  Per component:
 *           s = p + sigm * sigm;  kx = p / s;  kv = q / s;  y = z - x;  x = x + kx * y;  v = v + kv * y;
 *           r = r - kv * q;  p = p - kx * p;  q = q - kx * q                                   (r reads the old q)
 *       box from x as in 3', obs = B bit for bit, vel = {v[0], v[1]}; score, hits, misses, confirmed as in step 6.
 *   7'. An unmatched track keeps its predicted x, v, p, q, r and box.
 *   8'. Birth from B.  x = z(B), v = 0, q = 0; h = B.h; e = (2 * sp) * h; g = (10 * sv) * h; p = {e * e, e * e, sa * sa, e * e},
 *       r = {g * g, g * g, sav * sav, g * g}; box = obs = B bit for bit.
 *   9'. Compaction moves a filter record with its track.
 * A matched detection has w, h > 0 by the overlap statements (iw, ih > 0 with a finite box).  A birth with h <= 0 gets a NaN / inf
 * aspect and from the next prediction on a NaN / inf box, which pairs with nothing (a NaN r is no pair): it ages out as step 7 says.
 * filter_in == filter_out (in place) and two distinct buffers both work, as for the state; records at index >= n of a table of
 * filter_out are left as they were; a stream with no frame in the call keeps its block (its first n records are copied).
 * The kernel is the `true` instantiation of the tracker's kernel template (the `false` one is the two ops above, unchanged): the
 * association passes are the same code.  A thread keeps its track's mean and velocity (x, v) in registers and the 12 covariance
 * numbers in a column of LDS of its own, 96 KB beside the association's 58 KB -- 154 of gfx950's 160 KB per workgroup; 40 more
 * registers do not fit beside the track record under the 128 a lane of a 1024-thread workgroup has.  At the compaction a thread
 * sends its record a component at a time through the box buffer: it reads its column in front of the barrier and writes its column
 * behind it.  No atomics, nothing spins, every barrier is reached by all threads on values they read alike.
 * Refused before any launch, naming the value: everything mscnn_tracks_update_streams_fwd refuses (a null stream_of only with more
 * than one stream), a null call, a size that is not sizeof(mscnn_tracks_kalman_call), a null track, a null filter, filter_in or
 * filter_out (each by its name), a motion other than MSCNN_TRACK_MOTION_NONE, a std that is NaN, not finite or <= 0, filter_in /
 * filter_out not 16-byte aligned, filter_in and filter_out overlapping without being equal, a filter buffer overlapping a state
 * buffer.
 * The check: tests/track_kalman_witness.py restates the steps in float64 numpy (bit for bit) and, independently, the textbook
 * eight-state form (F, H, Q, R, K = P H^T S^-1), which agrees with the decoupled form to rounding with cross terms exactly 0.  The
 * accuracy of the tracker was NOT evaluated: there are no labels here. */
#ifndef MSCNN_TRACK_KALMAN_PARAMS_DEFINED
#define MSCNN_TRACK_KALMAN_PARAMS_DEFINED
typedef struct { double std_position, std_velocity;                              /* x h: 1/20, 1/160 */
                 double std_aspect, std_aspect_velocity, std_aspect_measure;     /* 1e-2, 1e-5, 1e-1 */
                 int freeze_lost_height; /* 1 */ } mscnn_track_kalman_params;
#endif
typedef struct { double x[4], v[4], p[4], q[4], r[4]; } mscnn_track_kalman_record;      /* 160 bytes */
typedef struct { size_t size;      /* sizeof(mscnn_tracks_kalman_call), refused otherwise */
                 const mscnn_track_params* track;  const mscnn_track_kalman_params* filter;
                 int num_frames, num_slots, num_streams;  const int* stream_of;      /* HOST; NULL with one stream */
                 const void* pack_dev;  int cap;
                 const void* state_in;  void* state_out;
                 const void* filter_in; void* filter_out;      /* num_streams * num_slots * max_tracks records, 16-byte aligned */
                 int max_tracks;  int* track_ids_dev;  void* stream; } mscnn_tracks_kalman_call;
MSCNN_API size_t mscnn_tracks_kalman_state_bytes(int num_slots, int max_tracks);      /* 0: refused */
MSCNN_API int mscnn_tracks_update_kalman_fwd(const mscnn_tracks_kalman_call* call);

/* The tracker with the matching as a choice: the greedy walk of steps 4 and 5, or the optimal assignment that SORT, DeepSORT and
 * ByteTrack solve (lapjv(cost = 1 - IoU, extend_cost = True, cost_limit = 1 - thr), as ByteTrack calls it).  They differ exactly
 * where a tracker is hard, on boxes that overlap each other: tracks A, B and detections a, b with r(A, b) = 0.65, r(A, a) = 0.60,
 * r(B, b) = 0.50, r(B, a) = 0 -- the walk takes (A, b), B has nothing left and a starts a new id; the assignment takes (A, a) + (B, b).
 * One entry point, one call struct in the pattern of mscnn_tracks_kalman_call (`size` must be sizeof(mscnn_tracks_assign_call));
 * mscnn_track_params, mscnn_track_record, mscnn_tracks_kalman_call and the three ops above do not change.  call->filter NULL: the
 * motion of call->track (none / linear), the ten steps of mscnn_tracks_update_streams_fwd; otherwise the Kalman filter with
 * track->motion NONE, the steps of mscnn_tracks_update_kalman_fwd, and filter_in / filter_out as there.  call->assign:
 * MSCNN_TRACK_ASSIGN_GREEDY is, byte for byte, the existing op for the same arguments (the same kernel instantiation).
 * MSCNN_TRACK_ASSIGN_OPTIMAL gives steps 4 and 5 a second form; everything else -- H and L, the tracks that take part, r(i, j), the
 * eligibility r > thr, steps 1 - 3 and 6 - 10 -- is unchanged:
 *   4''. Pass 1 as an assignment.  A pair is matched only if matching it beats leaving both its ends unmatched: the pass finds a
 *       maximum-WEIGHT matching over the eligible pairs (not necessarily of maximum cardinality).  Integer weights make the optimum
 *       independent of summation order: q(x) = (int64)floor(x * 2^30), exact in double; w(i, j) = q(r(i, j)) - q(thr) + 1 >= 1 for
 *       an eligible pair, every other pair is absent.  Shortest augmenting paths with potentials, all in int64:
 *       Rows = the pass's a tracks in table order.  Columns = the pass's b detections in ascending j (the real columns), then one
 *       private dummy column per row.  A real column costs -w and exists for eligible pairs only; a row's own dummy costs 0 and no
 *       other row reaches it.  u (rows), v and p (columns) start at 0 and free.
 *       For every row x in ascending order that has at least one eligible pair (the others stay unmatched and cost no step):
 *       minv = +inf, way unset, used = false for every column; i0 = x, j0 = the virtual start.  Repeat, as ONE STEP:
 *           for every unused column c row i0 has a cost for: cur = cost(i0, c) - u[i0] - v[c]; cur < minv[c]: minv[c] = cur, way[c] = j0;
 *           delta = min minv over the unused columns, j1 its column -- the lowest column index among equals, real before dummy;
 *           u[x] += delta; every used c: u[p[c]] += delta, v[c] -= delta; every unused c with a finite minv: minv[c] -= delta;
 *           j1 is used, j0 = j1; stop if j1 is free, else i0 = p[j1].
 *       Then augment back along way.  The matched pairs are the real columns that have a row.  A search takes at most min(a, b) + 1
 *       steps (every step uses a new assigned column or ends; the loop carries that bound), a pass at most a * (min(a, b) + 1).
 *   5''. Pass 2 (BYTE) likewise: the tracks of step 5 with every j in L, eligible iff r > match_thr_low, w with q(match_thr_low).
 * Header word MSCNN_TRACKS_STEPS (5) of a table: under OPTIMAL the table's running total of steps over both passes, read from
 * state_in, saturating at INT32_MAX, written to state_out; under GREEDY (and by the three ops above) it is written 0, as before.
 * mscnn_tracks_state_reset and _reset_slots zero it.  On sparse frames -- what is left behind an NMS -- most searches end after one or
 * two steps; a dense 1024 x 1024 table could take about 5 * 10^5.
 * The kernel: the tracker's kernel template has a second parameter, four instantiations; the two greedy ones are the code they were.
 * A thread is one row (its track), the real column of its detection and its row's dummy column; per step every thread does one
 * overlap and the workgroup one minimum of the key minv * 2048 + column (potentials stay under about 2^41, a column index takes 11
 * bits).  u, v, way, p and every track box lie in LDS arrays the greedy passes own and a pass leaves free (4 KB more for v's high
 * words, 128 bytes for the minimum).  Every loop exit is a value every thread reads out of LDS behind a barrier; nothing spins, no
 * atomics, no workgroup waits on another.
 * Refused before any launch, naming the value: everything the corresponding existing op refuses (under the name
 * tracks_update_assign; a null stream_of only with more than one stream), a null call, a size that is not
 * sizeof(mscnn_tracks_assign_call), an assign outside {1, 2}, filter_in or filter_out given without filter.
 * The check: tests/track_assign_witness.py restates 4'' in Python integers (bit for bit: ids, state, word 5, filter table) and is
 * held to an exhaustive search and to scipy's linear_sum_assignment.  The accuracy of the tracker was NOT evaluated: there are no
 * labels here. */
enum { MSCNN_TRACK_ASSIGN_GREEDY = 1, MSCNN_TRACK_ASSIGN_OPTIMAL = 2 };
typedef struct { size_t size;      /* sizeof(mscnn_tracks_assign_call), refused otherwise */
                 const mscnn_track_params* track;
                 const mscnn_track_kalman_params* filter;      /* NULL: the motion of track; else the Kalman filter, track->motion NONE */
                 int assign;                                   /* MSCNN_TRACK_ASSIGN_* */
                 int num_frames, num_slots, num_streams;  const int* stream_of;      /* HOST; NULL with one stream */
                 const void* pack_dev;  int cap;
                 const void* state_in;  void* state_out;
                 const void* filter_in; void* filter_out;      /* with filter only: as mscnn_tracks_kalman_call; NULL otherwise */
                 int max_tracks;  int* track_ids_dev;  void* stream; } mscnn_tracks_assign_call;
MSCNN_API int mscnn_tracks_update_assign_fwd(const mscnn_tracks_assign_call* call);

/* The render stage: the `show` block at the end of the reference's demo scripts (examples/kitti_car/run_mscnn_detection.m,
 * examples/caltech/run_mscnn_detection.m, examples/widerface/run_cascademscnn.m:136-150: every box with score >= show_thr drawn on
 * the frame, its score at the top edge) for the frames of a multi pack, in one device pass: outlines, an optional fill, labels
 * (score, track id) and an optional pixelation of the boxes' interiors (the face nets' use: anonymise a frame before it leaves the
 * machine).  Out of place: frame b is read from src_rgb[b] and its annotated copy written to dst_rgb[b], both uint8
 * [org_h[b]][org_w[b]][3] (RGB), every frame of its own size.  EVERY byte of every dst frame is written (a copy of src where nothing
 * is painted) and no other byte; src, the pack and the ids are only read.
 * The pack is the multi pack every final-stage op writes, mscnn_multi_pack_layout_of(num_frames * num_slots, cap); segment t * K + k
 * (K = num_slots) is slot k of frame t, its rows found by the rule of mscnn_tracks_update_fwd's step 2: entry {count, rows, row0, 0};
 * row offset = row0, unless K >= 2 and the entries of the frame's slots 0 and 1 hold the same row0 (the shared-row0 form of
 * mscnn_detections_multi_fwd), then K * row0 + k * rows.  A segment with count < 0, a negative offset or offset + count > cap is
 * empty.  Rows are [x y w h score] doubles in the frame's own pixels, as the scripts hand them to rectangle().  track_ids_dev[cap]
 * (mscnn_tracks_update_fwd's output: one id per pack row, <= 0 = no confirmed track) may be NULL when nothing asks for an id.
 * From the rounding on the semantics are integers only:
 *   Footprint of a row.  L = floor(x + .5), T = floor(y + .5), R = floor((x + w) + .5) - 1, Bt = floor((y + h) + .5) - 1, in double.
 *     A row is NOT DRAWN when !(score >= show_thr); when one of its five values is not finite; when |x|, |y|, |w| or |h| exceeds 2^30;
 *     when R < L or Bt < T; or when its box [L, R] x [T, Bt] holds no pixel of the frame (then it has no label either).  Otherwise
 *     clipping to the frame is implicit: pixels outside the frame do not exist.
 *   Paint order within a frame.  Slots in ascending k; within a slot the rows in DESCENDING index, so that row 0, the best score, is
 *     painted last and lies on top.  A pixel starts as the source pixel and takes from every drawn row, in that order:
 *     (a) pixelate = P > 0 and the pixel inside the box: the value BECOMES the rounded mean (sum + n / 2) / n, per channel, of the
 *         SOURCE frame over the pixel's block.  Blocks are P x P, anchored at (L, T) -- block (i, j) covers columns [L + i P,
 *         L + i P + P) and rows [T + j P, T + j P + P) -- and clipped to the box and to the frame; n = the pixels left.  This
 *         discards whatever earlier rows painted at that pixel (their outlines and labels too): the mosaic shows the source only.
 *     (b) fill_alpha > 0 and the pixel inside the box: v = blend(v, col, fill_alpha).
 *     (c) thickness > 0 and the pixel inside the box and less than `thickness` pixels from one of its four edges (px - L, R - px,
 *         py - T or Bt - py < thickness): v = blend(v, col, outline_alpha).
 *     (d) the pixel inside the row's label rectangle: v = col, opaque; a glyph pixel takes the ink instead, black (0, 0, 0) when
 *         299 r + 587 g + 114 b >= 128000 for col = (r, g, b) and white (255, 255, 255) otherwise.
 *     blend(v, c, a) = (v * (256 - a) + c * a + 128) >> 8 per channel.
 *   Colour.  color_by 0: colors[k % num_colors].  color_by 1: colors[id % num_colors] when the row's id > 0, else the slot's colour.
 *   Label text.  The score prints as the scripts' %.2f: c = floor(score * 100 + .5) clamped to [0, 100], "0.NN" or "1.00".  The id
 *     prints as its decimal digits.  label 1: the score.  label 2: the id; a row with id <= 0 has no label.  label 3: "ID 0.NN", one
 *     blank cell between the two; a row with id <= 0 has the score alone.
 *   Label geometry.  A character is a cell of 6 x 8 (w x h) pixels, each magnified to label_scale x label_scale; the 5 x 7 glyph sits
 *     in the cell's columns 1 .. 5 and rows 1 .. 7 (column 0 and row 0 stay blank).  The rectangle is chars * 6 * scale wide and
 *     8 * scale high.  Its bottom row is T - 1 and its left column L; if that puts its top row above the frame (< 0), its top row is
 *     T instead (inside the box); if its right end is past the frame's right edge, it is shifted left to end there, but not below
 *     column 0.  The bitmaps (csrc/render_glyphs.h) were drawn for this project; mscnn_render_glyph_rows(ch, rows) returns the seven
 *     rows of '0' .. '9', '.' or ' ' (bit 4 = the left column) and refuses every other ch.
 * One launch per 32 frames, the frame table by value in the arguments, no workspace, no host read.  Parallel over PIXELS: a workgroup
 * of 256 threads owns a 64 x 16 tile of a frame; its threads walk the frame's rows in paint order, 256 at a time, keep those whose
 * box or label rectangle meets the tile -- compacted in order into LDS by ballots and popcounts --, and every pixel then walks that
 * short list; chunk after chunk, so the order holds across chunks.  With pixelate on a pixel first looks for the LAST row of the chunk
 * that pixelates it and starts there (what earlier rows painted is discarded anyway): one mean per pixel and chunk, read straight
 * from the source.  Every loop bound and every value that guards a barrier is a kernel argument or a pack word clamped against cap, the
 * same in every thread: a garbage pack draws garbage boxes but lengthens no loop past num_slots * cap rows and moves no read outside
 * the pack or the ids.  No atomics, nothing spins, no workgroup waits on another; byte stores only (alignment 1).
 * Refused before any launch, naming the value: a null params / src_rgb / dst_rgb / org_h / org_w / pack_dev, a null frame pointer
 * (with its index), num_frames < 1, num_slots < 1, cap < 1 (or num_frames * num_slots * cap past 2^31 - 1), a frame size <= 0 or
 * above 2^30, thickness outside [0, 64], an alpha outside [0, 256], label outside [0, 3], label_scale outside [1, 8], color_by
 * outside {0, 1}, pixelate 1, negative or above 64, num_colors outside [1, 32], a NaN show_thr, label >= 2 or color_by 1 with a null
 * track_ids_dev, pack_dev not 16-byte aligned, track_ids_dev not 4-byte aligned, a dst frame that overlaps a src frame or another
 * dst frame (in place is refused too).
 * No pin on the reference: MATLAB's rectangle() and text() draw through the figure's renderer, nothing a kernel could be held to
 * bit for bit.  The check is tests/render_witness.py, a numpy restatement of the rules above with plain loops, byte for byte.  The
 * look of the glyphs and of the palette is a matter of taste that no test judges. */
#ifndef MSCNN_RENDER_PARAMS_DEFINED
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
enum { MSCNN_RENDER_FRAMES_PER_LAUNCH = 32 };
/* Alignment: pack_dev 16, track_ids_dev 4 (refused); frames 1. */
MSCNN_API int mscnn_render_detections_u8(const mscnn_render_params* p,
        const unsigned char* const* src_rgb /* HOST array of num_frames device pointers */,
        unsigned char* const* dst_rgb       /* HOST array of num_frames device pointers */,
        const int* org_h, const int* org_w, int num_frames, int num_slots,
        const void* pack_dev, int cap, const int* track_ids_dev /* [cap] or NULL */, void* stream);
MSCNN_API int mscnn_render_glyph_rows(int ch, unsigned char rows[7]);

/* The proposal half of the scripts' result (run_mscnn_detection.m:75-91, `final_proposals{k}`) for every image of a batched forward
 * in one pass.  props [R_all][6] = BoxOutput's proposals_score, rows [img x1 y1 x2 y2 score] grouped by image in ascending order;
 * desc[num_images], one per image.  Per image, in the script's types and order: w = x2 - x1, h = y2 - y1 in fp32 (no + 1); a row
 * stays iff score >= proposal_thr && w != 0 && h != 0 -- the very predicate the final stage applies to the same rows (a NaN score
 * goes, -0.0 is zero, a negative extent stays); kept rows go to double and THEN x / ratio_w, w / ratio_w, y / ratio_h, h / ratio_h in
 * double (unlike the final stage, which divides in fp32: there the script divides before its double()).  Kept rows keep their input
 * order (BoxOutput's: by score within an image); their places come from a ballot / popcount prefix, never from atomics.
 * pack_dev: the multi pack above with one slot per image (mscnn_multi_pack_layout_of(num_images, cap), cap >= R_all):
 *   [int32 num_images, R_all, cap, 0][num_images x int32 {count, rows, row0, 0}][cap x 5 doubles x y w h score][cap x int32 row]
 * image i owns pack rows [row0_i, row0_i + rows_i) and fills the first count_i; the int column is the ROI row relative to row0_i.
 * Every word of header and table is written by the kernel, rows of a slot past its count are left as they were.  One launch per
 * MSCNN_PROPOSALS_IMAGES_PER_LAUNCH images, one workgroup per image, no workspace, no host read, any number of rows per image.
 * Refused before any launch, naming the value: null pointers, num_images < 1, R_all < 1, cap < R_all, a NaN or non-positive ratio,
 * a NaN proposal_thr (and a props pointer that is not 8-byte aligned).  This stage has no pin on the reference: its check is a numpy
 * restatement written from the script. */
enum { MSCNN_PROPOSALS_IMAGES_PER_LAUNCH = 64 };
typedef struct { float proposal_thr; double ratio_h, ratio_w; } mscnn_proposals_desc;
MSCNN_API size_t mscnn_proposals_multi_pack_bytes(int num_images, int cap);
/* Alignment: props 8, pack_dev 16 (refused). */
MSCNN_API int mscnn_proposals_multi_fwd(const mscnn_proposals_desc* desc, int num_images, const float* props, int R_all, void* pack_dev,
                                        int cap, void* stream);

/* Caller-supplied ROIs: R rows become the two blobs BoxOutput would have written -- rois [R][5] = (image, x1, y1, x2, y2) and
 * props [R][6] = the same plus the score (props may be NULL: a BoxOutput with one top) -- in one launch, checked on the device
 * because the rows may live there.  Two input forms:
 *   MSCNN_ROIS_NET    fp32 rows [image x1 y1 x2 y2 score] in net-input coordinates, the layout of proposals_score: copied bit for bit.
 *   MSCNN_ROIS_IMAGE  double rows [image x y w h score] in original-image pixels with a 0-based image index, the row convention of
 *                     mscnn_net_proposals_multi; ratio_h / ratio_w: host arrays [num_images] (net input size / original image size):
 *                       x1 = (float)(x * ratio_w)          y1 = (float)(y * ratio_h)
 *                       x2 = (float)((x + w) * ratio_w)    y2 = (float)((y + h) * ratio_h)
 *                     sums and products in double, each result rounded to fp32 once; image and score are (float) of the double.
 *                     At most MSCNN_ROIS_MAX_RATIO_IMAGES images (the ratios travel with the launch); ratio_h / ratio_w are not read
 *                     in the NET form and may be NULL there.
 * Every row must hold finite values only (in the IMAGE form the fp32 results too), an image index that is a whole number in
 * [0, num_images), and an image index not smaller than the row's in front of it: rows are grouped by image, as BoxOutput emits them
 * (box_output_layer.cpp:107,156) and every reader of the blobs assumes.  An image may have no rows.
 * Outputs: image_rows [num_images] = rows of each image (written only when every row is good) and status [4] =
 *   {1, -1, 0, 0}                          every row is good, rois / props / image_rows are complete
 *   {0, first bad row, reason, 0}          reason: MSCNN_ROIS_BAD_* below, the first that applies to that row in their order
 * One workgroup walks the rows in steps of 256 and stops at the first bad row's verdict: the rows of the steps in front of that
 * row's step have been written, no row of its step and none behind it; bad input never makes the kernel read or write outside
 * its operands.  status and image_rows are written with ordinary stores and never read: they may be host-coherent pinned memory
 * (the caller then needs no copy: an event behind the launch, and the words are there).
 * Refused before the launch, naming the argument: a null rows / rois / image_rows / status, a coords value that is neither form,
 * R < 1, num_images < 1, a rows pointer that is not 8-byte aligned (the other pointers: 4), in the IMAGE form null ratios, more
 * images than the limit, a ratio that is not a positive finite number.  No pin on the reference (it has no such entry): the check
 * is a numpy restatement of the formulas above. */
enum { MSCNN_ROIS_NET = 0, MSCNN_ROIS_IMAGE = 1 };
enum { MSCNN_ROIS_BAD_NONFINITE = 1, MSCNN_ROIS_BAD_IMAGE = 2, MSCNN_ROIS_BAD_ORDER = 3 };
enum { MSCNN_ROIS_MAX_RATIO_IMAGES = 128 };
MSCNN_API const char* mscnn_rois_reason_text(int reason);
/* Alignment: rows 8 (refused); rois, props, image_rows, status 4. */
MSCNN_API int mscnn_rois_ingest_f32(const void* rows, int coords, int R, int num_images, const double* ratio_h, const double* ratio_w,
                                    float* rois, float* props, int* image_rows, int* status, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Image pre-processing in front of net.forward -- MATLAB `run_mscnn_detection.m:64-69`:
 * imresize(uint8 image, [H W]) (bicubic, uint8 after each 1-D pass), RGB -> BGR, single, subtract the
 * per-channel mean, hand to the net as its (1,3,H,W) input blob.
 * img_rgb: device uint8 [org_h][org_w][3] (row-major HWC, as any image decoder delivers it);
 * out: device float [3][H][W] (planes B, G, R); mean_bgr: host float[3] ({104,117,123} in the reference).
 * ------------------------------------------------------------------------------------------ */
MSCNN_API size_t mscnn_preprocess_workspace_bytes(int org_h, int org_w, int H, int W);
/* Alignment: workspace 16 (refused); img_rgb 1, out 4. */
MSCNN_API int mscnn_preprocess_u8_f32(const unsigned char* img_rgb, int org_h, int org_w, float* out, int H, int W,
                            const float* mean_bgr, void* workspace, size_t workspace_bytes, void* stream);
/* The same for a batch of `count` frames, each of its own size: imgs_rgb is a HOST array of `count` device pointers (frame b:
 * uint8 [org_h[b]][org_w[b]][3]); out: device float [count][3][H][W] (frame b in slice b).  Every slice is bit-identical to
 * mscnn_preprocess_u8_f32 on that frame.  Two launches per 32 frames.  The workspace holds every frame's intermediate at a
 * 256-byte aligned offset, back to back: mscnn_preprocess_batch_workspace_bytes returns that size (0 for arguments the op refuses).
 * Null pointers, count < 1, a size <= 0 or a too small workspace are refused before any launch. */
MSCNN_API size_t mscnn_preprocess_batch_workspace_bytes(int count, const int* org_h, const int* org_w, int H, int W);
/* Alignment: workspace 16 (refused); frames 1, out 4. */
MSCNN_API int mscnn_preprocess_batch_u8_f32(const unsigned char* const* imgs_rgb, const int* org_h, const int* org_w, int count,
                                  float* out, int H, int W, const float* mean_bgr, void* workspace, size_t workspace_bytes,
                                  void* stream);
/* VIEWS of uploaded frames as the images of one batch: a frame and its mirror, the tiles of a frame too large for one forward.
 * frames_rgb: a HOST array of num_frames device pointers (frame f: uint8 [org_h[f]][org_w[f]][3]); view v reads the window
 * [y0, y0 + h) x [x0, x0 + w) of frame views[v].frame, reversed along x when flip_x, and writes slice v of out [count][3][H][W].
 * Definition: slice v is bit-identical to mscnn_preprocess_u8_f32 on a contiguous copy of that window (mirrored with [:, ::-1] when
 * flip_x) -- the resize mirrors at the WINDOW's borders, the pass order (smaller scale first) is decided by the window's size, and no
 * pixel outside the window is ever read.  No copy of the window is made: its offset, the frame's row pitch (org_w * 3 bytes) and the
 * mirrored column are part of the first pass's source index; the second pass reads the window's intermediate only.  Two launches
 * per 32 views, the table of a chunk travels as a kernel argument; any number of views may name the same frame.  The workspace holds
 * every view's intermediate at a 256-byte aligned offset, back to back: mscnn_preprocess_views_workspace_bytes returns that size (0
 * for arguments the op refuses: null views, count < 1, a size <= 0, an empty window).
 * Refused before any launch, naming the value: null pointers (a null frame included), count < 1, num_frames < 1, a frame of size
 * <= 0, a view's frame outside [0, num_frames), a window with w < 1 or h < 1 or one that is not inside its frame, a flip_x that is
 * neither 0 nor 1, H or W <= 0, a workspace that is too small or not 16-byte aligned.
 * No pin on the reference (its scripts pre-process whole frames only): the check is the single-frame op on a host copy of the window
 * and a numpy restatement (tests/views_witness.py). */
#ifndef MSCNN_PREPROCESS_VIEW_DEFINED
#define MSCNN_PREPROCESS_VIEW_DEFINED
typedef struct { int frame; int x0, y0, w, h; int flip_x; } mscnn_preprocess_view;
#endif
MSCNN_API size_t mscnn_preprocess_views_workspace_bytes(const mscnn_preprocess_view* views, int count, int H, int W);
/* Alignment: workspace 16 (refused); frames 1, out 4. */
MSCNN_API int mscnn_preprocess_views_u8_f32(const unsigned char* const* frames_rgb, const int* org_h, const int* org_w, int num_frames,
                                            const mscnn_preprocess_view* views, int count, float* out, int H, int W,
                                            const float* mean_bgr, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* MSCNN_HIP_H_ */
