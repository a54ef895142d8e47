// DecodeBBox and the final detection stage for gfx950: one list (mscnn_detections_*_fwd), every segment of a batched forward in one
// pass (mscnn_detections_*multi*_fwd) and the tiled path for a list of more than kMaxK rows.  The device functions they are made of
// are det_device.h's; the candidate adds, the merge and Soft-NMS over them are det_candidates.hip, det_merge.hip and det_soft.hip.
//
// DecodeBBox: DecodeBBoxLayer<Dtype>::Forward_cpu (decode_bbox_layer.cpp:54-123) +
//   DecodeBBoxesWithPrior (math_functions.cpp:46-75), TEST phase (no filtering).  CPU-only in the
//   reference (decode_bbox_layer.hpp:41-42).
#include <cfloat>
#include <cmath>
#include <cstring>
#include "det_device.h"
#include "nms_large.h"

namespace {
using namespace mscnn_dev;

__global__ __launch_bounds__(256) void decode_bbox_kernel(const float* __restrict__ bbox, const float* __restrict__ prior,
                                                          float* __restrict__ out, int R, int bbox_dim, float m0, float m1,
                                                          float m2, float m3, float s0, float s1, float s2, float s3) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= R) return;
  const float xmin = prior[i * 5 + 1], ymin = prior[i * 5 + 2], xmax = prior[i * 5 + 3], ymax = prior[i * 5 + 4];
  const float pw = xmax - xmin + 1, ph = ymax - ymin + 1;
  const float cx = (float)(0.5 * (double)(xmax + xmin)), cy = (float)(0.5 * (double)(ymax + ymin));
  const float* b = bbox + (size_t)i * bbox_dim + 4;          // class 1 columns (decode_bbox_layer.cpp:116)
  const float bx = b[0] * s0 + m0, by = b[1] * s1 + m1, bw = b[2] * s2 + m2, bh = b[3] * s3 + m3;
  float tx = bx * pw + cx, ty = by * ph + cy;
  const float tw = pw * expf_libm(bw), th = ph * expf_libm(bh);
  tx -= (tw - 1) / 2; ty -= (th - 1) / 2;
  out[i * 5 + 0] = prior[i * 5];
  out[i * 5 + 1] = tx; out[i * 5 + 2] = ty; out[i * 5 + 3] = tx + tw - 1; out[i * 5 + 4] = ty + th - 1;
}

static_assert(DC_BIG_WORDS == BIG_STATE_WORDS, "cnt[DC_BIG ...] holds the tiled path's state words (nms_large.h)");

// Per-row transform + filter, key sort, write sorted boxes: the body of one workgroup (kSortThreads threads).  *n_out = survivors.
// (shared by det_transform_sort_kernel and the segmented det_seg_transform_sort_kernel: one code path, the same bits)
template <bool kThr>
__device__ __forceinline__ void det_transform_sort(const DetArgs& a, DetBox* __restrict__ sbox, double* __restrict__ sprob,
                                                   int* __restrict__ ssrc, DetBox* __restrict__ tmp_box, float* __restrict__ tmp_prob,
                                                   int* __restrict__ n_out) {
  __shared__ u64 sk[kSortCap];
  __shared__ int s_fill;
  const int tid = threadIdx.x;
  if (tid == 0) s_fill = 0;
  __syncthreads();
  for (int r = tid; r < a.R; r += kSortThreads) {
    DetBox b;
    float prob;
    if (!det_row<kThr>(a, r, &b, &prob)) continue;
    tmp_box[r] = b;
    tmp_prob[r] = prob;
    const int pos = atomicAdd(&s_fill, 1);
    if (pos < kMaxK) sk[pos] = det_key(prob, r);
  }
  __syncthreads();
  const int n = min(s_fill, kMaxK);
  if (tid == 0) *n_out = n;
  if (n == 0) return;
  int P = 1;
  while (P < n) P <<= 1;
  for (int i = n + tid; i < P; i += kSortThreads) sk[i] = 0ull;
  __syncthreads();
  bitonic_desc(sk, P, tid, kSortThreads);
  for (int i = tid; i < n; i += kSortThreads) {
    const int r = det_key_row(sk[i]);
    sbox[i] = tmp_box[r];
    sprob[i] = (double)tmp_prob[r];
    ssrc[i] = r;
  }
}

// One workgroup: the whole list.
__global__ __launch_bounds__(kSortThreads) void det_transform_sort_kernel(DetArgs a, DetBox* __restrict__ sbox,
                                                                          double* __restrict__ sprob, int* __restrict__ ssrc,
                                                                          DetBox* __restrict__ tmp_box,
                                                                          float* __restrict__ tmp_prob, int* __restrict__ cnt) {
  det_transform_sort<false>(a, sbox, sprob, ssrc, tmp_box, tmp_prob, cnt + DC_N);
}
__global__ __launch_bounds__(kSortThreads) void det_transform_sort_thr_kernel(DetArgs a, DetBox* __restrict__ sbox,
                                                                              double* __restrict__ sprob, int* __restrict__ ssrc,
                                                                              DetBox* __restrict__ tmp_box,
                                                                              float* __restrict__ tmp_prob, int* __restrict__ cnt) {
  det_transform_sort<true>(a, sbox, sprob, ssrc, tmp_box, tmp_prob, cnt + DC_N);
}

// ---- more than kMaxK rows (nms_large.h): the same three steps over HBM-resident lists -------------------------------------------
// The key kernel of the single list (det_tiled_of): keys[r] = the row's key, or 0 (padding, sorts last) when it is filtered out;
// cnt[DC_N] counts the survivors
__global__ __launch_bounds__(256) void det_transform_big_kernel(DetArgs a, u64* __restrict__ keys, DetBox* __restrict__ tmp_box,
                                                                float* __restrict__ tmp_prob, int* __restrict__ cnt) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= a.R) return;
  DetBox b;
  float prob;
  if (!det_row<false>(a, r, &b, &prob)) return;   // keys[] was cleared (the tiled path runs with the default nms params only)
  tmp_box[r] = b;
  tmp_prob[r] = prob;
  keys[r] = det_key(prob, r);
  atomicAdd(&cnt[DC_N], 1);
}

// the sorted list out of the sorted keys: row r of the caller's box / prob, its id tag[r] (tag == NULL: r itself)
__global__ __launch_bounds__(256) void det_gather_big_kernel(const u64* __restrict__ keys, const DetBox* __restrict__ box,
                                                             const float* __restrict__ prob, const int* __restrict__ tag,
                                                             DetBox* __restrict__ sbox, double* __restrict__ sprob,
                                                             int* __restrict__ ssrc, const int* __restrict__ cnt) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= cnt[DC_N]) return;
  const int r = det_key_row(keys[i]);
  sbox[i] = box[r];
  sprob[i] = (double)prob[r];
  ssrc[i] = tag ? tag[r] : r;
}

__global__ __launch_bounds__(256) void det_emit_big_kernel(const int* __restrict__ kept_idx, const int* __restrict__ state,
                                                           const DetBox* __restrict__ sbox, const double* __restrict__ sprob,
                                                           const int* __restrict__ ssrc, double* __restrict__ dets,
                                                           int* __restrict__ ids, int* __restrict__ count_out) {
  const int nk = state[BIG_NKEPT];
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row == 0) count_out[0] = nk;
  if (row >= nk) return;
  const int k = kept_idx[row];
  const DetBox b = sbox[k];
  double* d = dets + 5 * (size_t)row;
  d[0] = b.x; d[1] = b.y; d[2] = b.w; d[3] = b.h; d[4] = sprob[k];
  if (ids) ids[row] = ssrc[k];
}

__global__ __launch_bounds__(256) void det_mask_kernel(const DetBox* __restrict__ boxes, const int* __restrict__ cnt,
                                                       double overlap, u64* __restrict__ mask, int wpr) {
  det_mask_block<false>(boxes, cnt[DC_N], overlap, mask, wpr, blockIdx.y, blockIdx.x);
}
__global__ __launch_bounds__(256) void det_mask_min_kernel(const DetBox* __restrict__ boxes, const int* __restrict__ cnt,
                                                           double overlap, u64* __restrict__ mask, int wpr) {
  det_mask_block<true>(boxes, cnt[DC_N], overlap, mask, wpr, blockIdx.y, blockIdx.x);
}

__global__ __launch_bounds__(256) void det_scan_emit_kernel(const u64* __restrict__ mask, int wpr,
                                                            const DetBox* __restrict__ sbox, const double* __restrict__ sprob,
                                                            const int* __restrict__ ssrc, double* __restrict__ dets,
                                                            int* __restrict__ ids, const int* __restrict__ cnt,
                                                            int* __restrict__ count_out) {
  extern __shared__ __attribute__((aligned(16))) u64 dyn_lds[];
  det_scan_emit(mask, wpr, cnt[DC_N], sbox, sprob, ssrc, dets, ids, count_out, dyn_lds);
}

__global__ __launch_bounds__(256) void det_color_emit_kernel(const u64* __restrict__ mask, int wpr,
                                                             const DetBox* __restrict__ sbox, const double* __restrict__ sprob,
                                                             const int* __restrict__ ssrc, double* __restrict__ dets,
                                                             int* __restrict__ ids, const int* __restrict__ cnt,
                                                             int* __restrict__ count_out) {
  extern __shared__ __attribute__((aligned(16))) u64 dyn_lds[];
  det_color_emit(mask, wpr, cnt[DC_N], sbox, sprob, ssrc, dets, ids, count_out, dyn_lds);
}

// ---- every segment of a batched forward in one pass (mscnn_detections_multi_fwd, mscnn_detections_cascade_multi_fwd) ----------------
// With K slots per image and C classes per source (DetSource, det_device.h), segment s = image s / K, source (s % K) / C, slot
// k = s % K (image-major, then source, then class).  Each segment finds its [row0, row0 + rows) in ITS source's props by binary
// search on the device and runs the single-list path's three bodies above on that range, in a workspace slice of its own (max_rows
// rows, det_slice_of).  Its detections go to pack rows [K row0 + k rows, + rows): a slot it places without knowing any other
// segment; all slots tile [0, K R_all).
struct DetSegArgs {
  int R_all, slots_per_image, classes_per_source, max_rows, wpr, cap, num_segs, s0;       // s0: first segment of this launch
  char* ws; size_t seg_stride_box, seg_stride_mask;                     // workspace: per-segment slices (det_slice_of)
  DetPack pack;                                                         // header + table, dets, ids (mscnn_multi_pack_layout)
  DetNms nms;                                                           // one setting per call (mscnn_nms_params)
  DetSource src[kCascadeMaxOutputs];
  DetSeg seg[kSegsPerLaunch];
};
static_assert(sizeof(DetSegArgs) <= 4096, "DetSegArgs travels as kernel arguments");
enum { SEG_N = 0, SEG_ROW0 = 1, SEG_ROWS = 2, SEG_BAD = 3 };   // the segment's kSliceWords workspace words
__device__ __forceinline__ DetSlice det_seg_slice(const DetSegArgs& a, int s) {
  return det_slice_of<true>(a.ws, a.num_segs, a.max_rows, a.seg_stride_box, a.seg_stride_mask, s);
}

// one workgroup per segment: find the rows, transform + filter + sort them
template <bool kThr>
__device__ __forceinline__ void det_seg_transform_sort(const DetSegArgs& a) {
  const int j = blockIdx.x, s = a.s0 + j;
  const int img = s / a.slots_per_image;
  const DetSource& t = a.src[(s % a.slots_per_image) / a.classes_per_source];
  const DetSlice p = det_seg_slice(a, s);
  __shared__ int s_range[2];
  if (threadIdx.x < 2) s_range[threadIdx.x] = det_image_lower_bound(t.props, a.R_all, img + threadIdx.x, t.cascade ? 5 : 6);
  if (s == 0 && threadIdx.x == 0) {
    a.pack.hdr[0] = a.num_segs; a.pack.hdr[1] = a.R_all; a.pack.hdr[2] = a.cap; a.pack.hdr[3] = 0;
  }
  __syncthreads();
  const int row0 = s_range[0], rows = s_range[1] - s_range[0];
  // (more rows than the host-side bound the workspace is sized by: nothing is run, the table says so and the unpacker refuses it)
  const bool bad = rows > a.max_rows;
  if (threadIdx.x == 0) { p.cnt[SEG_ROW0] = row0; p.cnt[SEG_ROWS] = rows; p.cnt[SEG_BAD] = bad ? 1 : 0; }
  if (bad) { if (threadIdx.x == 0) p.cnt[SEG_N] = 0; return; }
  const DetArgs d = det_args_of(t, a.seg[j], row0, rows, a.nms);
  det_transform_sort<kThr>(d, p.sbox, p.sprob, p.ssrc, p.tbox, p.tprob, p.cnt + SEG_N);
}
__global__ __launch_bounds__(kSortThreads) void det_seg_transform_sort_kernel(DetSegArgs a) { det_seg_transform_sort<false>(a); }
__global__ __launch_bounds__(kSortThreads) void det_seg_transform_sort_thr_kernel(DetSegArgs a) { det_seg_transform_sort<true>(a); }

// grid (wpr, wpr, segments): blocks past a segment's own n exit at once
template <bool kDnmMin>
__device__ __forceinline__ void det_seg_mask(const DetSegArgs& a) {
  const int j = blockIdx.z, s = a.s0 + j;
  const DetSlice p = det_seg_slice(a, s);
  det_mask_block<kDnmMin>(p.sbox, p.cnt[SEG_N], a.seg[j].nms_overlap, p.mask, a.wpr, blockIdx.y, blockIdx.x);
}
__global__ __launch_bounds__(256) void det_seg_mask_kernel(DetSegArgs a) { det_seg_mask<false>(a); }
__global__ __launch_bounds__(256) void det_seg_mask_min_kernel(DetSegArgs a) { det_seg_mask<true>(a); }

// one workgroup per segment: greedy scan (kGreedy) or column-OR, emit into the segment's slot, its table entry
// {count (-1: rows over the bound), rows, row0, 0}
template <bool kGreedy>
__device__ __forceinline__ void det_seg_emit(const DetSegArgs& a, u64* dyn_lds) {
  const int j = blockIdx.x, s = a.s0 + j;
  const DetSlice p = det_seg_slice(a, s);
  const int row0 = p.cnt[SEG_ROW0], rows = p.cnt[SEG_ROWS];
  int* ent = a.pack.hdr + MSCNN_MULTI_PACK_WORDS * (size_t)(1 + s);
  if (threadIdx.x == 0) { ent[1] = rows; ent[2] = row0; ent[3] = 0; }
  if (p.cnt[SEG_BAD]) { if (threadIdx.x == 0) ent[0] = -1; return; }
  const size_t slot = mscnn_multi_pack_slot(a.slots_per_image, row0, s % a.slots_per_image, rows);
  if (kGreedy) det_scan_emit(p.mask, a.wpr, p.cnt[SEG_N], p.sbox, p.sprob, p.ssrc, a.pack.dets + 5 * slot, a.pack.ids + slot, ent, dyn_lds);
  else det_color_emit(p.mask, a.wpr, p.cnt[SEG_N], p.sbox, p.sprob, p.ssrc, a.pack.dets + 5 * slot, a.pack.ids + slot, ent, dyn_lds);
}
__global__ __launch_bounds__(256) void det_seg_scan_emit_kernel(DetSegArgs a) {
  extern __shared__ __attribute__((aligned(16))) u64 dyn_lds[];
  det_seg_emit<true>(a, dyn_lds);
}
__global__ __launch_bounds__(256) void det_seg_color_emit_kernel(DetSegArgs a) {
  extern __shared__ __attribute__((aligned(16))) u64 dyn_lds[];
  det_seg_emit<false>(a, dyn_lds);
}

// the single list's workspace (mscnn_detections_workspace_bytes)
struct DetLayout { size_t cnt, sbox, sprob, ssrc, tbox, tprob, mask, keys, rinit, kidx, kbox, total; int wpr, sortP; bool big; };
DetLayout det_layout(int R) {
  DetLayout L;
  const int n = R < 1 ? 1 : R;
  L.big = n > kMaxK;                         // more rows than the LDS-resident path holds: sort in HBM, tiled NMS
  L.wpr = L.big ? kTileWords : (n + 63) / 64;
  L.sortP = L.big ? big_sort_pow2(n) : 0;
  size_t o = 0;
  L.cnt = o; o += 256;                       // [DC_N ...] and, at DC_BIG, the tiled path's state words
  L.sbox = o; o += det_al((size_t)n * sizeof(DetBox));
  L.sprob = o; o += det_al((size_t)n * sizeof(double));
  L.ssrc = o; o += det_al((size_t)n * sizeof(int));
  L.tbox = o; o += det_al((size_t)n * sizeof(DetBox));
  L.tprob = o; o += det_al((size_t)n * sizeof(float));
  L.mask = o; o += det_al((size_t)(L.big ? kMaxK : n) * L.wpr * sizeof(u64));
  L.keys = o; o += L.big ? det_al((size_t)L.sortP * sizeof(u64)) : 0;
  L.rinit = o; o += L.big ? det_al(64 * sizeof(u64)) : 0;
  L.kidx = o; o += L.big ? det_al((size_t)n * sizeof(int)) : 0;
  L.kbox = o; o += L.big ? det_al((size_t)n * sizeof(DetBox)) : 0;
  L.total = o;
  return L;
}
}  // namespace

using namespace mscnn;

// ---- the tiled path and the source checks the other files of the stage call (det_device.h) --------------------------------------------
namespace mscnn_dev {

DetTiled det_tiled_of(void* workspace, int kcap) {
  const DetLayout L = det_layout(kcap);
  char* ws = static_cast<char*>(workspace);
  return DetTiled{reinterpret_cast<u64*>(ws + L.keys), L.sortP, reinterpret_cast<int*>(ws + L.cnt), reinterpret_cast<DetBox*>(ws + L.tbox),
                  reinterpret_cast<float*>(ws + L.tprob)};
}

void det_tiled_gather(const u64* keys, const DetBox* box, const float* prob, const int* tag, DetBox* sbox, double* sprob, int* ssrc,
                      const int* cnt, int kcap, hipStream_t st) {
  det_gather_big_kernel<<<cdiv(kcap, 256), 256, 0, st>>>(keys, box, prob, tag, sbox, sprob, ssrc, cnt);
}

int det_tiled_nms(void* workspace, int kcap, const DetBox* box, const float* prob, const int* tag, double overlap, double* dets,
                  int* ids, int* count_out, hipStream_t st) {
  const DetLayout L = det_layout(kcap);
  char* ws = static_cast<char*>(workspace);
  int* cnt = reinterpret_cast<int*>(ws + L.cnt);
  DetBox* sbox = reinterpret_cast<DetBox*>(ws + L.sbox);
  double* sprob = reinterpret_cast<double*>(ws + L.sprob);
  int* ssrc = reinterpret_cast<int*>(ws + L.ssrc);
  u64* mask = reinterpret_cast<u64*>(ws + L.mask);
  u64* keys = reinterpret_cast<u64*>(ws + L.keys);
  int* kidx = reinterpret_cast<int*>(ws + L.kidx);
  MSCNN_HIP_TRY(big_sort_desc(keys, L.sortP, st));
  det_gather_big_kernel<<<cdiv(kcap, 256), 256, 0, st>>>(keys, box, prob, tag, sbox, sprob, ssrc, cnt);
  MSCNN_POST_LAUNCH();
  auto launch_mask = [&](const DetBox* tile, const int* tile_n) {
    det_mask_kernel<<<dim3(kTileWords, kTileWords), 256, 0, st>>>(tile, tile_n, overlap, mask, kTileWords);
  };
  MSCNN_HIP_TRY((big_nms_tiles<DetTr>(sbox, cnt + DC_N, 0, kcap, DetTr::Params{overlap}, mask, reinterpret_cast<u64*>(ws + L.rinit), kidx,
                                      reinterpret_cast<DetBox*>(ws + L.kbox), cnt + DC_BIG, launch_mask, st)));
  det_emit_big_kernel<<<cdiv(kcap, 256), 256, 0, st>>>(kidx, cnt + DC_BIG, sbox, sprob, ssrc, dets, ids, count_out);
  MSCNN_POST_LAUNCH();
  return MSCNN_OK;
}

int det_plain_source(const char* name, const mscnn_detections_desc* desc, int S, const float* bbox_pred, const float* cls_pred,
                     const float* props, DetSource* src) {
  const int ncls = desc[0].ncls;
  for (int s = 0; s < S; ++s)
    MSCNN_REQUIRE(desc[s].ncls == ncls && desc[s].cls_id >= 1 && desc[s].cls_id <= ncls && ncls >= 2, "%s: segment %d: cls_id %d of %d", name, s,
                  desc[s].cls_id, desc[s].ncls);
  *src = DetSource{bbox_pred, cls_pred, props, ncls, 0};
  return MSCNN_OK;
}

int det_cascade_sources(const char* name, const mscnn_detections_desc* desc, int num_images, int num_outputs, int num_classes,
                        const mscnn_cascade_output* outputs, DetSource* src) {
  for (int o = 0; o < num_outputs; ++o) {
    MSCNN_REQUIRE(outputs[o].boxes && outputs[o].cls_prob && outputs[o].props, "%s: output %d of %d: null pointer", name, o, num_outputs);
    MSCNN_REQUIRE(outputs[o].ncls >= 2, "%s: output %d: %d probability columns", name, o, outputs[o].ncls);
  }
  const int K = num_outputs * num_classes;
  MSCNN_REQUIRE((long)num_images * K <= (long)(1 << 24), "%s: %d images x %d outputs x %d classes", name, num_images, num_outputs, num_classes);
  const int S = num_images * K;
  for (int s = 0; s < S; ++s) {
    const int o = (s % K) / num_classes;
    MSCNN_REQUIRE(desc[s].cls_id >= 1 && desc[s].cls_id <= outputs[o].ncls, "%s: segment %d (output %d): cls_id %d of %d", name, s, o,
                  desc[s].cls_id, outputs[o].ncls);
  }
  for (int o = 0; o < num_outputs; ++o) src[o] = DetSource{outputs[o].boxes, outputs[o].cls_prob, outputs[o].props, outputs[o].ncls, 1};
  return MSCNN_OK;
}

}  // namespace mscnn_dev

extern "C" int mscnn_decodebbox_fwd_f32(const float* bbox, const float* prior, float* out, int R, int bbox_dim,
                                        const float* mean_host, const float* std_host, void* stream) {
  MSCNN_REQUIRE(R >= 0, "decodebbox: R < 0");
  MSCNN_REQUIRE(bbox_dim == 8, "decodebbox: bbox channels must be 8 (decode_bbox_layer.cpp:47), got %d", bbox_dim);
  if (R == 0) return MSCNN_OK;
  MSCNN_REQUIRE(bbox && prior && out && mean_host && std_host, "decodebbox: null pointer");
  for (int k = 0; k < 4; ++k)      // decode_bbox_layer.cpp:30 (CHECK_GT: a NaN fails it too)
    MSCNN_REQUIRE(std_host[k] > 0.f, "decodebbox: bbox_std[%d] = %g must be > 0", k, (double)std_host[k]);
  decode_bbox_kernel<<<cdiv(R, 256), 256, 0, as_stream(stream)>>>(bbox, prior, out, R, bbox_dim, mean_host[0], mean_host[1],
                                                                  mean_host[2], mean_host[3], std_host[0], std_host[1],
                                                                  std_host[2], std_host[3]);
  MSCNN_POST_LAUNCH();
  return MSCNN_OK;
}

extern "C" size_t mscnn_detections_workspace_bytes(int R) { return det_layout(R).total; }

// NULL -> the defaults; every field checked, the offending value named.  *out is written whole (padding included: zero).
extern "C" int mscnn_nms_params_resolve(const mscnn_nms_params* nms, mscnn_nms_params* out) {
  MSCNN_REQUIRE(out, "nms params: null output");
  mscnn_nms_params r;
  std::memset(&r, 0, sizeof(r));
  r.type = MSCNN_NMS_TYPE_MAXG; r.ovr_dnm = MSCNN_NMS_OVR_UNION; r.thr = -HUGE_VAL; r.det_thr = 0.f;
  if (nms) {
    MSCNN_REQUIRE(nms->type != MSCNN_NMS_TYPE_MS, "nms params: type %d ('ms') is not supported: it needs nonMaxSuprList", nms->type);
    MSCNN_REQUIRE(nms->type != MSCNN_NMS_TYPE_COVER, "nms params: type %d ('cover') is not supported: its scores come from a BLAS "
                  "mat-vec whose summation order is not pinned", nms->type);
    MSCNN_REQUIRE(nms->type != MSCNN_NMS_TYPE_NONE, "nms params: type %d ('none') is not supported: read the rows without a final stage",
                  nms->type);
    MSCNN_REQUIRE(nms->type == MSCNN_NMS_TYPE_MAXG || nms->type == MSCNN_NMS_TYPE_MAX, "nms params: type %d (0 = 'maxg', 1 = 'max')",
                  nms->type);
    MSCNN_REQUIRE(nms->ovr_dnm == MSCNN_NMS_OVR_UNION || nms->ovr_dnm == MSCNN_NMS_OVR_MIN,
                  "nms params: ovr_dnm %d (0 = 'union', 1 = 'min')", nms->ovr_dnm);
    MSCNN_REQUIRE(!(nms->thr != nms->thr), "nms params: thr is NaN");
    MSCNN_REQUIRE(nms->det_thr >= 0.f && nms->det_thr <= FLT_MAX, "nms params: det_thr %g (0 = off, else a finite positive probability)",
                  (double)nms->det_thr);
    r.type = nms->type; r.ovr_dnm = nms->ovr_dnm; r.thr = nms->thr; r.det_thr = nms->det_thr;
  }
  *out = r;
  return MSCNN_OK;
}
// bbNms's own spelling of the knobs (type / ovrDnm strings, thr, maxn) -> mscnn_nms_params; NULL strings: the defaults
extern "C" int mscnn_nms_params_from_names(const char* type, const char* ovr_dnm, double thr, double maxn, float det_thr,
                                           mscnn_nms_params* out) {
  MSCNN_REQUIRE(out, "nms params: null output");
  mscnn_nms_params r;
  std::memset(&r, 0, sizeof(r));
  const char* const types[] = {"maxg", "max", "ms", "cover", "none"};
  r.type = -1;
  for (int k = 0; k < 5; ++k) if (!type ? k == 0 : std::strcmp(type, types[k]) == 0) r.type = k;
  MSCNN_REQUIRE(r.type >= 0, "nms params: unknown type '%s' ('maxg' or 'max')", type);
  r.ovr_dnm = !ovr_dnm || std::strcmp(ovr_dnm, "union") == 0 ? MSCNN_NMS_OVR_UNION : std::strcmp(ovr_dnm, "min") == 0 ? MSCNN_NMS_OVR_MIN : -1;
  MSCNN_REQUIRE(r.ovr_dnm >= 0, "nms params: unknown ovr_dnm '%s' ('union' or 'min')", ovr_dnm);
  MSCNN_REQUIRE(maxn == HUGE_VAL, "nms params: maxn %g: only maxn = inf (bbNms's default, no split-and-recurse) is supported", maxn);
  r.thr = thr; r.det_thr = det_thr;
  return mscnn_nms_params_resolve(&r, out);
}
static bool nms_is_default(const mscnn_nms_params& r) {
  return r.type == MSCNN_NMS_TYPE_MAXG && r.ovr_dnm == MSCNN_NMS_OVR_UNION && r.thr == -HUGE_VAL && r.det_thr == 0.f;
}

static int detections_launch(const mscnn_detections_desc* desc, int cascade, float det_thr, const mscnn_nms_params* nms_in,
                             const float* bbox_pred, const float* cls_pred, const float* props, int R, double* dets_out, int* ids_out,
                             int* count_out_dev, void* workspace, size_t workspace_bytes, void* stream) {
  mscnn_nms_params nms;
  if (int rc = mscnn_nms_params_resolve(nms_in, &nms)) return rc;
  MSCNN_REQUIRE(!cascade || nms.det_thr == 0.f, "detections: nms params det_thr %g is the plain stage's: the cascade stage takes its "
                "det_thr as an argument", (double)nms.det_thr);
  MSCNN_REQUIRE(desc && count_out_dev && workspace, "detections: null pointer");
  MSCNN_REQUIRE_ALIGNED(workspace, 16, "detections: workspace");
  MSCNN_REQUIRE_ALIGNED(dets_out, 8, "detections: dets_out");
  MSCNN_REQUIRE(R >= 0, "detections: R < 0");
  MSCNN_REQUIRE(desc->ncls >= 2 && desc->cls_id >= 1 && desc->cls_id <= desc->ncls, "detections: cls_id %d of %d",
                desc->cls_id, desc->ncls);
  const DetLayout L = det_layout(R);
  if (workspace_bytes < L.total) {
    set_error("detections: workspace %zu < %zu", workspace_bytes, L.total);
    return MSCNN_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  char* ws = static_cast<char*>(workspace);
  int* cnt = reinterpret_cast<int*>(ws + L.cnt);
  // (cnt needs no clearing: det_transform_sort_kernel writes cnt[DC_N] unconditionally before anything reads it)
  if (R == 0) {
    MSCNN_HIP_TRY(hipMemsetAsync(count_out_dev, 0, sizeof(int), st));
    return MSCNN_OK;
  }
  MSCNN_REQUIRE(bbox_pred && cls_pred && props && dets_out, "detections: null pointer");
  DetBox* sbox = reinterpret_cast<DetBox*>(ws + L.sbox);
  double* sprob = reinterpret_cast<double*>(ws + L.sprob);
  int* ssrc = reinterpret_cast<int*>(ws + L.ssrc);
  DetBox* tbox = reinterpret_cast<DetBox*>(ws + L.tbox);
  float* tprob = reinterpret_cast<float*>(ws + L.tprob);
  u64* mask = reinterpret_cast<u64*>(ws + L.mask);
  DetArgs a;
  a.bbox_pred = bbox_pred; a.cls_pred = cls_pred; a.props = props;
  a.R = R; a.ncls = desc->ncls; a.cls_id = desc->cls_id;
  for (int k = 0; k < 4; ++k) { a.mean[k] = desc->bbox_mean[k]; a.stdv[k] = desc->bbox_std[k]; }
  a.proposal_thr = cascade ? det_thr : desc->proposal_thr;
  a.cascade = cascade;
  a.nms_thr = nms.thr; a.det_thr = cascade ? 0.f : nms.det_thr;
  // MATLAB: single op double -> single (the double operand is converted to single first)
  a.ratio_h = (float)desc->ratio_h; a.ratio_w = (float)desc->ratio_w;
  a.org_h = (float)desc->org_h; a.org_w = (float)desc->org_w;
  if (L.big) {
    // (the tiled path of nms_large.h is the greedy scan over union overlaps, tile after tile)
    MSCNN_REQUIRE(nms_is_default(nms), "detections: %d rows > %d run the tiled path, which has the default nms params only (got type %d, "
                  "ovr_dnm %d, thr %g, det_thr %g)", R, kMaxK, nms.type, nms.ovr_dnm, nms.thr, (double)nms.det_thr);
    const DetTiled w = det_tiled_of(workspace, R);
    MSCNN_HIP_TRY(hipMemsetAsync(w.cnt, 0, 256, st));
    MSCNN_HIP_TRY(hipMemsetAsync(w.keys, 0, (size_t)w.P * sizeof(u64), st));
    det_transform_big_kernel<<<cdiv(R, 256), 256, 0, st>>>(a, w.keys, w.tbox, w.tprob, w.cnt);
    MSCNN_POST_LAUNCH();
    return det_tiled_nms(workspace, R, w.tbox, w.tprob, nullptr, desc->nms_overlap, dets_out, ids_out, count_out_dev, st);
  }
  // (the default setting runs the three kernels it always ran; thr / det_thr, 'min' and 'max' each swap one of them)
  if (nms_has_thr(nms)) det_transform_sort_thr_kernel<<<1, kSortThreads, 0, st>>>(a, sbox, sprob, ssrc, tbox, tprob, cnt);
  else det_transform_sort_kernel<<<1, kSortThreads, 0, st>>>(a, sbox, sprob, ssrc, tbox, tprob, cnt);
  MSCNN_POST_LAUNCH();
  if (nms.ovr_dnm == MSCNN_NMS_OVR_MIN) det_mask_min_kernel<<<dim3(L.wpr, L.wpr), 256, 0, st>>>(sbox, cnt, desc->nms_overlap, mask, L.wpr);
  else det_mask_kernel<<<dim3(L.wpr, L.wpr), 256, 0, st>>>(sbox, cnt, desc->nms_overlap, mask, L.wpr);
  MSCNN_POST_LAUNCH();
  const size_t lds = (size_t)2 * 64 * L.wpr * sizeof(u64);
  if (nms.type == MSCNN_NMS_TYPE_MAXG)
    det_scan_emit_kernel<<<1, 256, lds, st>>>(mask, L.wpr, sbox, sprob, ssrc, dets_out, ids_out, cnt, count_out_dev);
  else
    det_color_emit_kernel<<<1, 256, lds, st>>>(mask, L.wpr, sbox, sprob, ssrc, dets_out, ids_out, cnt, count_out_dev);
  MSCNN_POST_LAUNCH();
  return MSCNN_OK;
}

extern "C" int mscnn_detections_fwd(const mscnn_detections_desc* desc, const float* bbox_pred, const float* cls_pred,
                                    const float* props, int R, double* dets_out, int* ids_out, int* count_out_dev,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  return detections_launch(desc, 0, 0.f, nullptr, bbox_pred, cls_pred, props, R, dets_out, ids_out, count_out_dev, workspace,
                           workspace_bytes, stream);
}

extern "C" int mscnn_detections_nms_fwd(const mscnn_detections_desc* desc, const mscnn_nms_params* nms, const float* bbox_pred,
                                        const float* cls_pred, const float* props, int R, double* dets_out, int* ids_out,
                                        int* count_out_dev, void* workspace, size_t workspace_bytes, void* stream) {
  return detections_launch(desc, 0, 0.f, nms, bbox_pred, cls_pred, props, R, dets_out, ids_out, count_out_dev, workspace,
                           workspace_bytes, stream);
}

extern "C" int mscnn_detections_cascade_fwd(const mscnn_detections_desc* desc, float det_thr, const float* boxes,
                                            const float* cls_prob, const float* props, int R, double* dets_out, int* ids_out,
                                            int* count_out_dev, void* workspace, size_t workspace_bytes, void* stream) {
  return detections_launch(desc, 1, det_thr, nullptr, boxes, cls_prob, props, R, dets_out, ids_out, count_out_dev, workspace,
                           workspace_bytes, stream);
}

extern "C" int mscnn_detections_cascade_nms_fwd(const mscnn_detections_desc* desc, float det_thr, const mscnn_nms_params* nms,
                                                const float* boxes, const float* cls_prob, const float* props, int R, double* dets_out,
                                                int* ids_out, int* count_out_dev, void* workspace, size_t workspace_bytes, void* stream) {
  return detections_launch(desc, 1, det_thr, nms, boxes, cls_prob, props, R, dets_out, ids_out, count_out_dev, workspace,
                           workspace_bytes, stream);
}

// ---- all segments in one pass ----------------------------------------------------------------------------------------------------------
extern "C" size_t mscnn_detections_multi_pack_bytes(int num_segments, int cap) {
  return mscnn_multi_pack_layout_of(num_segments, cap).total;
}

extern "C" size_t mscnn_detections_multi_workspace_bytes(int num_segments, int max_rows_per_image) {
  if (num_segments < 1 || max_rows_per_image > kMaxK) return 0;
  return det_slices_bytes(num_segments, max_rows_per_image, true);
}
extern "C" size_t mscnn_detections_cascade_multi_workspace_bytes(int num_segments, int max_rows_per_image) {
  return mscnn_detections_multi_workspace_bytes(num_segments, max_rows_per_image);
}

// desc[num_images * num_sources * C] (validated by the caller, as the workspace is): carve the pack, three launches per 32 segments
static int det_seg_launch(const DetSource* src, int num_sources, const mscnn_detections_desc* desc, float det_thr,
                          const mscnn_nms_params& nms, int num_images, int C, int R_all, int M, void* pack_dev, int cap, void* workspace,
                          void* stream) {
  hipStream_t st = as_stream(stream);
  const int S = num_images * num_sources * C;
  DetSegArgs a = {};
  a.R_all = R_all; a.slots_per_image = num_sources * C; a.classes_per_source = C; a.max_rows = M; a.wpr = (M + 63) / 64; a.cap = cap;
  a.num_segs = S;
  a.nms = det_nms_of(nms);
  a.ws = static_cast<char*>(workspace);
  a.seg_stride_box = det_slice_box_bytes(M, true); a.seg_stride_mask = det_slice_mask_bytes(M);
  for (int o = 0; o < num_sources; ++o) a.src[o] = src[o];
  a.pack = det_pack_of(pack_dev, S, cap);
  for (int s0 = 0; s0 < S; s0 += kSegsPerLaunch) {
    const int ns = S - s0 < kSegsPerLaunch ? S - s0 : kSegsPerLaunch;
    a.s0 = s0;
    for (int j = 0; j < ns; ++j) a.seg[j] = det_seg_of(desc[s0 + j], src[0].cascade, det_thr);
    if (nms_has_thr(nms)) det_seg_transform_sort_thr_kernel<<<ns, kSortThreads, 0, st>>>(a);
    else det_seg_transform_sort_kernel<<<ns, kSortThreads, 0, st>>>(a);
    MSCNN_POST_LAUNCH();
    if (nms.ovr_dnm == MSCNN_NMS_OVR_MIN) det_seg_mask_min_kernel<<<dim3(a.wpr, a.wpr, ns), 256, 0, st>>>(a);
    else det_seg_mask_kernel<<<dim3(a.wpr, a.wpr, ns), 256, 0, st>>>(a);
    MSCNN_POST_LAUNCH();
    const size_t lds = (size_t)2 * 64 * a.wpr * sizeof(u64);
    if (nms.type == MSCNN_NMS_TYPE_MAXG) det_seg_scan_emit_kernel<<<ns, 256, lds, st>>>(a);
    else det_seg_color_emit_kernel<<<ns, 256, lds, st>>>(a);
    MSCNN_POST_LAUNCH();
  }
  return MSCNN_OK;
}

extern "C" int mscnn_detections_multi_nms_fwd(const mscnn_detections_desc* desc, const mscnn_nms_params* nms_in, int num_images,
                                              int num_classes, const float* bbox_pred, const float* cls_pred, const float* props,
                                              int R_all, int max_rows_per_image, void* pack_dev, int cap, void* workspace,
                                              size_t workspace_bytes, void* stream) {
  mscnn_nms_params nms;
  if (int rc = mscnn_nms_params_resolve(nms_in, &nms)) return rc;
  MSCNN_REQUIRE(desc && pack_dev && workspace, "detections_multi: null pointer");
  MSCNN_REQUIRE_ALIGNED(pack_dev, 16, "detections_multi: pack_dev");
  MSCNN_REQUIRE_ALIGNED(workspace, 16, "detections_multi: workspace");
  MSCNN_REQUIRE(num_images >= 1 && num_classes >= 1, "detections_multi: %d images x %d classes", num_images, num_classes);
  MSCNN_REQUIRE(R_all >= 1 && bbox_pred && cls_pred && props, "detections_multi: R_all = %d (BoxOutput emits at least one row)", R_all);
  MSCNN_REQUIRE(max_rows_per_image >= 1 && max_rows_per_image <= kMaxK,
                "detections_multi: %d rows per image > %d: run mscnn_detections_fwd per segment", max_rows_per_image, kMaxK);
  MSCNN_REQUIRE((long)num_classes * R_all <= (long)cap, "detections_multi: pack capacity %d < %d classes x %d ROIs", cap, num_classes,
                R_all);
  const int S = num_images * num_classes;
  DetSource src;
  if (int rc = det_plain_source("detections_multi", desc, S, bbox_pred, cls_pred, props, &src)) return rc;
  const size_t need = mscnn_detections_multi_workspace_bytes(S, max_rows_per_image);
  if (workspace_bytes < need) {
    set_error("detections_multi: workspace %zu < %zu", workspace_bytes, need);
    return MSCNN_ERR_WORKSPACE;
  }
  return det_seg_launch(&src, 1, desc, 0.f, nms, num_images, num_classes, R_all, max_rows_per_image, pack_dev, cap, workspace, stream);
}

extern "C" int mscnn_detections_multi_fwd(const mscnn_detections_desc* desc, int num_images, int num_classes, const float* bbox_pred,
                                          const float* cls_pred, const float* props, int R_all, int max_rows_per_image, void* pack_dev,
                                          int cap, void* workspace, size_t workspace_bytes, void* stream) {
  return mscnn_detections_multi_nms_fwd(desc, nullptr, num_images, num_classes, bbox_pred, cls_pred, props, R_all, max_rows_per_image,
                                        pack_dev, cap, workspace, workspace_bytes, stream);
}

extern "C" int mscnn_detections_cascade_multi_nms_fwd(const mscnn_detections_desc* desc, float det_thr, const mscnn_nms_params* nms_in,
                                                      int num_images, int num_outputs, int num_classes,
                                                      const mscnn_cascade_output* outputs, int R_all, int max_rows_per_image,
                                                      void* pack_dev, int cap, void* workspace, size_t workspace_bytes, void* stream) {
  const char* name = "detections_cascade_multi";
  mscnn_nms_params nms;
  if (int rc = mscnn_nms_params_resolve(nms_in, &nms)) return rc;
  MSCNN_REQUIRE(nms.det_thr == 0.f, "%s: nms params det_thr %g is the plain stage's: the cascade stage takes its det_thr as an argument", name,
                (double)nms.det_thr);
  MSCNN_REQUIRE(num_outputs >= 1 && num_outputs <= kCascadeMaxOutputs, "%s: %d cascade outputs (1 .. %d)", name, num_outputs,
                kCascadeMaxOutputs);
  MSCNN_REQUIRE(desc && outputs && pack_dev && workspace, "%s: null pointer", name);
  MSCNN_REQUIRE_ALIGNED(pack_dev, 16, "detections_cascade_multi: pack_dev");
  MSCNN_REQUIRE_ALIGNED(workspace, 16, "detections_cascade_multi: workspace");
  MSCNN_REQUIRE(num_images >= 1 && num_classes >= 1, "%s: %d images x %d classes", name, num_images, num_classes);
  MSCNN_REQUIRE(R_all >= 1, "%s: R_all = %d (BoxOutput emits at least one row)", name, R_all);
  // (the bounds of this entry point in front of what it checks about its sources like the candidate adds)
  MSCNN_REQUIRE(max_rows_per_image >= 1 && max_rows_per_image <= kMaxK, "%s: %d rows per image > %d: run mscnn_detections_cascade_fwd per segment",
                name, max_rows_per_image, kMaxK);
  const int K = num_outputs * num_classes;
  MSCNN_REQUIRE((long)K * R_all <= (long)cap, "%s: pack capacity %d < %d outputs x %d classes x %d ROIs", name, cap, num_outputs, num_classes,
                R_all);
  DetSource src[kCascadeMaxOutputs];
  if (int rc = det_cascade_sources(name, desc, num_images, num_outputs, num_classes, outputs, src)) return rc;
  const size_t need = mscnn_detections_cascade_multi_workspace_bytes(num_images * K, max_rows_per_image);
  if (workspace_bytes < need) {
    set_error("%s: workspace %zu < %zu", name, workspace_bytes, need);
    return MSCNN_ERR_WORKSPACE;
  }
  return det_seg_launch(src, num_outputs, desc, det_thr, nms, num_images, num_classes, R_all, max_rows_per_image, pack_dev, cap, workspace,
                        stream);
}

extern "C" int mscnn_detections_cascade_multi_fwd(const mscnn_detections_desc* desc, float det_thr, int num_images, int num_outputs,
                                                  int num_classes, const mscnn_cascade_output* outputs, int R_all,
                                                  int max_rows_per_image, void* pack_dev, int cap, void* workspace,
                                                  size_t workspace_bytes, void* stream) {
  return mscnn_detections_cascade_multi_nms_fwd(desc, det_thr, nullptr, num_images, num_outputs, num_classes, outputs, R_all,
                                                max_rows_per_image, pack_dev, cap, workspace, workspace_bytes, stream);
}
