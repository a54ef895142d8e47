// DecodeBBox and the final detection stage for gfx950.
//
// DecodeBBox: DecodeBBoxLayer<Dtype>::Forward_cpu (decode_bbox_layer.cpp:54-123) +
//   DecodeBBoxesWithPrior (math_functions.cpp:46-75), TEST phase (no filtering).  CPU-only in the
//   reference (decode_bbox_layer.hpp:41-42).
// Final stage: the MATLAB post-processing of the net outputs, examples/kitti_car/run_mscnn_detection.m:75-120
//   + utils/bbNms.m:112-126 (nmsMax, greedy, union).  MATLAB semantics restated: single-precision
//   arithmetic until `double([...])`, stable descending sort on prob (ties: lower row first), IoU and
//   threshold test in double, pairs with iw <= 0 or ih <= 0 skipped.
// Same kernel structure as BoxOutput's NMS: parallel bit-matrix + one-wavefront greedy scan.
// bbNms's user knobs (mscnn_nms_params): ovrDnm = 'min' is another denominator in the bit matrix (bbNms.m:121), type = 'max' a
// column-OR of that matrix instead of the greedy scan (bbNms.m:117 with greedy = 0), thr the strict prob > thr of bbNms.m:85.
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>
#include "common.h"
#include "box_device.h"
#include "det_rows.h"
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

struct DetBox { double x, y, w, h; };

struct DetArgs {
  const float* bbox_pred; const float* cls_pred; const float* props;
  int R, ncls, cls_id;
  float mean[4], stdv[4];
  float proposal_thr, ratio_h, ratio_w, org_h, org_w;
  int cascade;        // 1: run_cascademscnn.m:84-117 -- bbox_pred = decoded boxes [R][5], cls_pred = in-net probabilities,
                      //    props = proposal rows [R][5]; proposal_thr = det_thr
  double nms_thr;     // bbNms's thr (bbNms.m:85, strict >); -inf by default
  float det_thr;      // plain stage only: examples/widerface/run_mscnn_detection.m:139-143 (> 0: rows with !(prob >= det_thr) go)
};

// mscnn_nms_params as the kernels take it (resolved: NULL -> the defaults)
struct DetNms { double thr; float det_thr; int type, ovr_dnm; };

enum { DC_N = 0, DC_WORDS = 4, DC_BIG = 4 /* + BIG_STATE_WORDS (nms_large.h) */ };

// One input row -> box and prob in MATLAB's types.  false: the row is filtered out.
// kThr: bbNms's thr / the plain det_thr are set (mscnn_nms_params); without them the default thr = -inf is the literal it always was,
// so the default kernels are the instructions they were before the params existed.
template <bool kThr>
__device__ __forceinline__ bool det_row(const DetArgs& a, int r, DetBox* box, float* prob_out) {
  if (a.cascade) {
    const float* q = a.props + 5 * (size_t)r;
    const float cw = q[3] - q[1] + 1.f, ch = q[4] - q[2] + 1.f;                      // run_cascademscnn.m:104
    if (!(cw != 0 && ch != 0)) return false;                                         // :107
    const float* t = a.bbox_pred + 5 * (size_t)r;
    float x1 = t[1] / a.ratio_w, x2 = t[3] / a.ratio_w;                              // :88-89
    float y1 = t[2] / a.ratio_h, y2 = t[4] / a.ratio_h;
    x1 = fmaxf(0.f, x1); y1 = fmaxf(0.f, y1);                                        // :91
    x2 = fminf(x2, a.org_w); y2 = fminf(y2, a.org_h);                                // :92
    const float w = x2 - x1 + 1.f, h = y2 - y1 + 1.f;                                // :93
    const float prob = a.cls_pred[(size_t)r * a.ncls + (a.cls_id - 1)];              // :113
    if (a.proposal_thr > 0 && !(prob >= a.proposal_thr)) return false;               // :115-117 (det_thr)
    if (kThr ? !((double)prob > a.nms_thr) : !(prob > -INFINITY)) return false;      // bbNms.m:85
    *box = DetBox{(double)x1, (double)y1, (double)w, (double)h};
    *prob_out = prob;
    return true;
  }
  const float* q = a.props + 6 * (size_t)r;
  const float px = q[1], py = q[2], pw = q[3] - q[1], ph = q[4] - q[2], sc = q[5];
  if (!det_keep_proposal(sc, pw, ph, a.proposal_thr)) return false;                  // :82 (det_rows.h: shared with proposals.hip)
  const float* bp = a.bbox_pred + (size_t)r * 4 * a.ncls + 4 * (a.cls_id - 1);      // :95
  float b0 = bp[0] * a.stdv[0], b1 = bp[1] * a.stdv[1], b2 = bp[2] * a.stdv[2], b3 = bp[3] * a.stdv[3];
  b0 += a.mean[0]; b1 += a.mean[1]; b2 += a.mean[2]; b3 += a.mean[3];
  const float* cp = a.cls_pred + (size_t)r * a.ncls;
  float se = 0.f;
  for (int k = 0; k < a.ncls; ++k) se += expf_libm(cp[k]);                           // :101-102
  const float prob = expf_libm(cp[a.cls_id - 1]) / se;
  const float ctr_x = px + 0.5f * pw, ctr_y = py + 0.5f * ph;
  float tx = b0 * pw + ctr_x, ty = b1 * ph + ctr_y;
  float tw = pw * expf_libm(b2), th = ph * expf_libm(b3);
  tx = tx - tw / 2.f; ty = ty - th / 2.f;
  tx = tx / a.ratio_w; tw = tw / a.ratio_w;
  ty = ty / a.ratio_h; th = th / a.ratio_h;
  tx = fmaxf(0.f, tx); ty = fmaxf(0.f, ty);
  tw = fminf(tw, a.org_w - tx); th = fminf(th, a.org_h - ty);
  if (kThr && a.det_thr > 0 && !(prob >= a.det_thr)) return false;                   // widerface/run_mscnn_detection.m:139-143
  if (kThr ? !((double)prob > a.nms_thr) : !(prob > -INFINITY)) return false;        // bbNms.m:85 (NaN drops out)
  *box = DetBox{(double)tx, (double)ty, (double)tw, (double)th};
  *prob_out = prob;
  return true;
}

// stable descending: larger prob first, then LOWER row first (never 0: orderable(x) > 0 for every x > -inf)
__device__ __forceinline__ u64 det_key(float prob, int r) {
  return ((u64)orderable(prob) << 32) | (u64)(0xffffffffu - (unsigned)r);
}

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
    const int r = (int)(0xffffffffu - (unsigned)(sk[i] & 0xffffffffull));
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
// keys[r] = the row's key, or 0 (padding, sorts last) when it is filtered out; cnt[DC_N] counts the survivors
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

__global__ __launch_bounds__(256) void det_gather_big_kernel(const u64* __restrict__ keys, const DetBox* __restrict__ tmp_box,
                                                             const float* __restrict__ tmp_prob, DetBox* __restrict__ sbox,
                                                             double* __restrict__ sprob, int* __restrict__ ssrc,
                                                             const int* __restrict__ cnt) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= cnt[DC_N]) return;
  const int r = (int)(0xffffffffu - (unsigned)(keys[i] & 0xffffffffull));
  sbox[i] = tmp_box[r];
  sprob[i] = (double)tmp_prob[r];
  ssrc[i] = r;
}

struct DetTr {
  typedef DetBox Box;
  struct Params { double overlap; };
  // == det_mask_kernel's test (A the earlier box): bbNms.m:117-124, all in double
  static __device__ __forceinline__ bool over(const DetBox& A, const DetBox& B, const Params& p) {
    const double iw = fmin(A.x + A.w, B.x + B.w) - fmax(A.x, B.x);
    if (iw <= 0) return false;
    const double ih = fmin(A.y + A.h, B.y + B.h) - fmax(A.y, B.y);
    if (ih <= 0) return false;
    double o = iw * ih;
    const double u = A.w * A.h + B.w * B.h - o;
    o = o / u;
    return o > p.overlap;
  }
};

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

// One 64 x 64 block (rb, cb) of the upper-triangular bit matrix over n sorted boxes.
// (256 threads per 64 x 64 block, the four waves split the columns -- as nms_mask_kernel of boxoutput.hip)
// kDnmMin: ovrDnm = 'min' -- the denominator is the smaller of the two areas instead of the union (bbNms.m:121).  (A template
// parameter: the union kernels keep the instructions they had.)
template <bool kDnmMin>
__device__ __forceinline__ void det_mask_block(const DetBox* __restrict__ boxes, int n, double overlap, u64* __restrict__ mask, int wpr,
                                               int rb, int cb) {
  if (cb < rb || rb * 64 >= n || cb * 64 >= n) return;
  __shared__ DetBox cbox[64];
  __shared__ unsigned part[4][64];
  const int t = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int j0 = cb * 64;
  if (wv == 0 && j0 + t < n) cbox[t] = boxes[j0 + t];
  __syncthreads();
  const int i = rb * 64 + t;
  unsigned bits = 0;
  if (i < n) {
    const DetBox A = boxes[i];
    const double as_a = A.w * A.h, xe_a = A.x + A.w, ye_a = A.y + A.h;
    const int jn = min(64, n - j0);
    for (int q = wv * 16; q < wv * 16 + 16; ++q) {
      if (q >= jn || j0 + q <= i) continue;
      const DetBox B = cbox[q];
      const double iw = fmin(xe_a, B.x + B.w) - fmax(A.x, B.x);
      if (iw <= 0) continue;
      const double ih = fmin(ye_a, B.y + B.h) - fmax(A.y, B.y);
      if (ih <= 0) continue;
      double o = iw * ih;
      const double u = kDnmMin ? fmin(as_a, B.w * B.h) : as_a + B.w * B.h - o;
      o = o / u;
      if (o > overlap) bits |= 1u << (q & 15);
    }
  }
  part[wv][t] = bits;
  __syncthreads();
  if (wv == 0 && i < n)
    mask[(size_t)i * wpr + cb] = (u64)part[0][t] | ((u64)part[1][t] << 16) | ((u64)part[2][t] << 32) | ((u64)part[3][t] << 48);
}

__global__ __launch_bounds__(256) void det_mask_kernel(const DetBox* __restrict__ boxes, const int* __restrict__ cnt,
                                                       double overlap, u64* __restrict__ mask, int wpr) {
  det_mask_block<false>(boxes, cnt[DC_N], overlap, mask, wpr, blockIdx.y, blockIdx.x);
}
__global__ __launch_bounds__(256) void det_mask_min_kernel(const DetBox* __restrict__ boxes, const int* __restrict__ cnt,
                                                           double overlap, u64* __restrict__ mask, int wpr) {
  det_mask_block<true>(boxes, cnt[DC_N], overlap, mask, wpr, blockIdx.y, blockIdx.x);
}

// Prefix count + emit of the keep words of n sorted boxes (lane c of wave 0 holds the keep word of boxes [64 c, 64 c + 64)) by one
// 256-thread workgroup: kept box number k lands in dets[k] / ids[k], the count in *count_out.
__device__ __forceinline__ void det_emit_kept(u64 mykeep, int n, const DetBox* __restrict__ sbox, const double* __restrict__ sprob,
                                              const int* __restrict__ ssrc, double* __restrict__ dets, int* __restrict__ ids,
                                              int* __restrict__ count_out) {
  __shared__ u64 keepw[64];
  __shared__ int pre[64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (wave == 0) {
    keepw[lane] = mykeep;
    const int mine = __popcll(mykeep);
    int incl = mine;
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_up(incl, d, 64);
      if (lane >= d) incl += v;
    }
    pre[lane] = incl - mine;
    if (lane == 63) count_out[0] = incl;
  }
  __syncthreads();
  for (int k = tid; k < n; k += 256) {
    const int c = k >> 6, l = k & 63;
    const u64 kw = keepw[c];
    if (!((kw >> l) & 1ull)) continue;
    const int row = pre[c] + __popcll(kw & ((1ull << l) - 1ull));
    const DetBox b = sbox[k];
    double* d = dets + 5 * (size_t)row;
    d[0] = b.x; d[1] = b.y; d[2] = b.w; d[3] = b.h; d[4] = sprob[k];
    if (ids) ids[row] = ssrc[k];
  }
}

// Greedy scan (type = 'maxg') + emit of n sorted boxes by one 256-thread workgroup.  dyn_lds: 2 * 64 * wpr u64.
__device__ __forceinline__ void det_scan_emit(const u64* __restrict__ mask, int wpr, int n, const DetBox* __restrict__ sbox,
                                              const double* __restrict__ sprob, const int* __restrict__ ssrc, double* __restrict__ dets,
                                              int* __restrict__ ids, int* __restrict__ count_out, u64* dyn_lds) {
  if (n <= 0) { if (threadIdx.x == 0) count_out[0] = 0; return; }
  const u64 mykeep = greedy_scan(mask, n, wpr, wpr, dyn_lds);
  det_emit_kept(mykeep, n, sbox, sprob, ssrc, dets, ids, count_out);
}

// type = 'max' (nmsMax with greedy = 0, bbNms.m:117-123): box j goes exactly when some i < j has bit (i, j) set, whether or not i
// itself went -- the OR of column j over the rows above it, no serial dependency.  Lane = word of the row (coalesced), wave w takes
// rows w, w + 4, ...; only words on or right of the diagonal block are read (the others were never written), rows >= n never.  The
// four partial ORs meet in the first 4 * wpr words of det_scan_emit's dynamic LDS (2 * 64 * wpr); then the same emit.
__device__ __forceinline__ void det_color_emit(const u64* __restrict__ mask, int wpr, int n, const DetBox* __restrict__ sbox,
                                               const double* __restrict__ sprob, const int* __restrict__ ssrc, double* __restrict__ dets,
                                               int* __restrict__ ids, int* __restrict__ count_out, u64* dyn_lds) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (n <= 0) { if (tid == 0) count_out[0] = 0; return; }
  const int nw = (n + 63) >> 6;                            // words in use (<= wpr <= 63)
  u64 acc = 0;
  if (lane < nw)
    for (int i = wave; i < n && (i >> 6) <= lane; i += 4) acc |= mask[(size_t)i * wpr + lane];
  if (lane < nw) dyn_lds[wave * wpr + lane] = acc;
  __syncthreads();
  u64 mykeep = 0;
  if (wave == 0 && lane < nw) {
    const u64 removed = (dyn_lds[lane] | dyn_lds[wpr + lane]) | (dyn_lds[2 * wpr + lane] | dyn_lds[3 * wpr + lane]);
    const int valid = min(64, n - lane * 64);
    mykeep = ~removed;
    if (valid < 64) mykeep &= (1ull << valid) - 1ull;
  }
  det_emit_kept(mykeep, n, sbox, sprob, ssrc, dets, ids, count_out);
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
// A source is a blob triple whose ROI rows are grouped by image, the image index in column 0 of props (box_output_layer.cpp:107,
// :156; DecodeBBox copies it, decode_bbox_layer.cpp:110).  The plain stage has one (bbox_pred / cls_pred / proposals_score,
// cascade = 0); the cascade stage one per cascade output (decoded boxes / probabilities / proposals, cascade = 1).  With K slots per
// image and C classes per source, segment s = image s / K, source (s % K) / C, slot k = s % K (image-major, then source, then class).
// Each segment finds its [row0, row0 + rows) in ITS source's props by binary search on the device and runs the single-list path's
// three bodies above on that range, in a workspace slice of its own (max_rows rows).  Its detections go to pack rows
// [K row0 + k rows, + rows): a slot it places without knowing any other segment; all slots tile [0, K R_all).
constexpr int kSegsPerLaunch = 32;         // sources and segment parameters travel as kernel arguments (2.3 KB of the 4 KB)
constexpr int kCascadeMaxOutputs = 4;
struct DetSource { const float* boxes; const float* cls; const float* props; int ncls, cascade; };   // row strides: props 6 / 5, boxes 4 ncls / 5
struct DetSeg { float mean[4], stdv[4]; float proposal_thr, ratio_h, ratio_w, org_h, org_w; int cls_id; double nms_overlap; };
struct DetSegArgs {
  int R_all, slots_per_image, classes_per_source, max_rows, wpr, cap, num_segs, s0;       // s0: first segment of this launch
  char* ws; size_t seg_stride_box, seg_stride_mask;                     // workspace: per-segment slices (det_multi_ptrs)
  int* hdr; double* dets; int* ids;                                     // pack: header + table, dets, ids (mscnn_multi_pack_layout)
  DetNms nms;                                                           // one setting per call (mscnn_nms_params)
  DetSource src[kCascadeMaxOutputs];
  DetSeg seg[kSegsPerLaunch];
};
static_assert(sizeof(DetSegArgs) <= 4096, "DetSegArgs travels as kernel arguments");
enum { SEG_N = 0, SEG_ROW0 = 1, SEG_ROWS = 2, SEG_BAD = 3, SEG_WORDS = 4 };   // workspace words per segment

struct DetMultiPtrs { int* cnt; DetBox* sbox; double* sprob; int* ssrc; DetBox* tbox; float* tprob; u64* mask; };
__device__ __forceinline__ DetMultiPtrs det_multi_ptrs(const DetSegArgs& a, int s) {
  // slices: [cnt: S x SEG_WORDS ints][sbox][sprob][ssrc][tbox][tprob] per segment (max_rows each, 256-byte aligned), then the masks
  const size_t M = (size_t)a.max_rows;
  char* base = a.ws + 256 * (((size_t)a.num_segs * SEG_WORDS * sizeof(int) + 255) / 256) + (size_t)s * a.seg_stride_box;
  DetMultiPtrs p;
  p.cnt = reinterpret_cast<int*>(a.ws) + (size_t)s * SEG_WORDS;
  const size_t a32 = (M * sizeof(DetBox) + 255) / 256 * 256, a8 = (M * sizeof(double) + 255) / 256 * 256,
               a4 = (M * sizeof(int) + 255) / 256 * 256;
  p.sbox = reinterpret_cast<DetBox*>(base);
  p.sprob = reinterpret_cast<double*>(base + a32);
  p.ssrc = reinterpret_cast<int*>(base + a32 + a8);
  p.tbox = reinterpret_cast<DetBox*>(base + a32 + a8 + a4);
  p.tprob = reinterpret_cast<float*>(base + 2 * a32 + a8 + a4);
  p.mask = reinterpret_cast<u64*>(a.ws + 256 * (((size_t)a.num_segs * SEG_WORDS * sizeof(int) + 255) / 256) +
                                  (size_t)a.num_segs * a.seg_stride_box + (size_t)s * a.seg_stride_mask);
  return p;
}

// one workgroup per segment: find the rows, transform + filter + sort them
template <bool kThr>
__device__ __forceinline__ void det_seg_transform_sort(const DetSegArgs& a) {
  const int j = blockIdx.x, s = a.s0 + j;
  const int img = s / a.slots_per_image;
  const DetSource& t = a.src[(s % a.slots_per_image) / a.classes_per_source];
  const int prop_stride = t.cascade ? 5 : 6, box_stride = t.cascade ? 5 : 4 * t.ncls;
  const DetMultiPtrs p = det_multi_ptrs(a, s);
  __shared__ int s_range[2];
  if (threadIdx.x < 2) s_range[threadIdx.x] = det_image_lower_bound(t.props, a.R_all, img + threadIdx.x, prop_stride);
  if (s == 0 && threadIdx.x == 0) {
    a.hdr[0] = a.num_segs; a.hdr[1] = a.R_all; a.hdr[2] = a.cap; a.hdr[3] = 0;
  }
  __syncthreads();
  const int row0 = s_range[0], rows = s_range[1] - s_range[0];
  // (more rows than the host-side bound the workspace is sized by: nothing is run, the table says so and the unpacker refuses it)
  const bool bad = rows > a.max_rows;
  if (threadIdx.x == 0) { p.cnt[SEG_ROW0] = row0; p.cnt[SEG_ROWS] = rows; p.cnt[SEG_BAD] = bad ? 1 : 0; }
  if (bad) { if (threadIdx.x == 0) p.cnt[SEG_N] = 0; return; }
  const DetSeg& g = a.seg[j];
  DetArgs d;
  d.bbox_pred = t.boxes + (size_t)row0 * box_stride; d.cls_pred = t.cls + (size_t)row0 * t.ncls; d.props = t.props + (size_t)row0 * prop_stride;
  d.R = rows; d.ncls = t.ncls; d.cls_id = g.cls_id;
  for (int k = 0; k < 4; ++k) { d.mean[k] = g.mean[k]; d.stdv[k] = g.stdv[k]; }
  d.proposal_thr = g.proposal_thr; d.ratio_h = g.ratio_h; d.ratio_w = g.ratio_w; d.org_h = g.org_h; d.org_w = g.org_w;
  d.cascade = t.cascade;
  d.nms_thr = a.nms.thr; d.det_thr = t.cascade ? 0.f : a.nms.det_thr;
  det_transform_sort<kThr>(d, p.sbox, p.sprob, p.ssrc, p.tbox, p.tprob, p.cnt + SEG_N);
}
__global__ __launch_bounds__(kSortThreads) void det_seg_transform_sort_kernel(DetSegArgs a) { det_seg_transform_sort<false>(a); }
__global__ __launch_bounds__(kSortThreads) void det_seg_transform_sort_thr_kernel(DetSegArgs a) { det_seg_transform_sort<true>(a); }

// grid (wpr, wpr, segments): blocks past a segment's own n exit at once
template <bool kDnmMin>
__device__ __forceinline__ void det_seg_mask(const DetSegArgs& a) {
  const int j = blockIdx.z, s = a.s0 + j;
  const DetMultiPtrs p = det_multi_ptrs(a, s);
  det_mask_block<kDnmMin>(p.sbox, p.cnt[SEG_N], a.seg[j].nms_overlap, p.mask, a.wpr, blockIdx.y, blockIdx.x);
}
__global__ __launch_bounds__(256) void det_seg_mask_kernel(DetSegArgs a) { det_seg_mask<false>(a); }
__global__ __launch_bounds__(256) void det_seg_mask_min_kernel(DetSegArgs a) { det_seg_mask<true>(a); }

// one workgroup per segment: greedy scan (kGreedy) or column-OR, emit into the segment's slot, its table entry
// {count (-1: rows over the bound), rows, row0, 0}
template <bool kGreedy>
__device__ __forceinline__ void det_seg_emit(const DetSegArgs& a, u64* dyn_lds) {
  const int j = blockIdx.x, s = a.s0 + j;
  const DetMultiPtrs p = det_multi_ptrs(a, s);
  const int row0 = p.cnt[SEG_ROW0], rows = p.cnt[SEG_ROWS];
  int* ent = a.hdr + MSCNN_MULTI_PACK_WORDS * (size_t)(1 + s);
  if (threadIdx.x == 0) { ent[1] = rows; ent[2] = row0; ent[3] = 0; }
  if (p.cnt[SEG_BAD]) { if (threadIdx.x == 0) ent[0] = -1; return; }
  const size_t slot = mscnn_multi_pack_slot(a.slots_per_image, row0, s % a.slots_per_image, rows);
  if (kGreedy) det_scan_emit(p.mask, a.wpr, p.cnt[SEG_N], p.sbox, p.sprob, p.ssrc, a.dets + 5 * slot, a.ids + slot, ent, dyn_lds);
  else det_color_emit(p.mask, a.wpr, p.cnt[SEG_N], p.sbox, p.sprob, p.ssrc, a.dets + 5 * slot, a.ids + slot, ent, dyn_lds);
}
__global__ __launch_bounds__(256) void det_seg_scan_emit_kernel(DetSegArgs a) {
  extern __shared__ __attribute__((aligned(16))) u64 dyn_lds[];
  det_seg_emit<true>(a, dyn_lds);
}
__global__ __launch_bounds__(256) void det_seg_color_emit_kernel(DetSegArgs a) {
  extern __shared__ __attribute__((aligned(16))) u64 dyn_lds[];
  det_seg_emit<false>(a, dyn_lds);
}

// ---- the candidates of several forwards of an image, merged before the NMS (mscnn_detections_candidates_*, mscnn_detections_merge_fwd) ----
// A segment's list: cand_cap slots of box / prob / tag and two ints {rows that wanted in, overflow flag}.  `add` runs the rows of one
// forward through det_row above -- the final stage's own row transform -- applies the forward's view in double and appends the
// survivors behind the list's count in row order; `merge` sorts each list by det_key(prob, candidate index) and runs the bit matrix
// and the scan / column-OR above over it.  One workgroup owns a segment's list in every kernel: no atomics on global memory, no
// workgroup waits on another, the order of a list is (order of the add calls, row) whatever the timing.
enum { CAND_WANTED = 0, CAND_OVER = 1, CAND_WORDS = 2 };
struct DetCand { int* cnt; DetBox* box; float* prob; int* tag; };      // cnt: CAND_WORDS ints per segment; the lists: cand_cap slots per segment
__host__ __device__ __forceinline__ size_t cand_al(size_t v) { return (v + 255) / 256 * 256; }
__host__ __device__ __forceinline__ size_t det_cand_bytes(int S, int cap) {
  const size_t n = (size_t)S * (size_t)cap;
  return cand_al((size_t)S * CAND_WORDS * sizeof(int)) + cand_al(n * sizeof(DetBox)) + 2 * cand_al(n * sizeof(int));
}
__host__ __device__ __forceinline__ DetCand det_cand_of(char* cand, int S, int cap) {
  const size_t n = (size_t)S * (size_t)cap;
  DetCand c;
  c.cnt = reinterpret_cast<int*>(cand);
  char* p = cand + cand_al((size_t)S * CAND_WORDS * sizeof(int));
  c.box = reinterpret_cast<DetBox*>(p); p += cand_al(n * sizeof(DetBox));
  c.prob = reinterpret_cast<float*>(p); p += cand_al(n * sizeof(float));
  c.tag = reinterpret_cast<int*>(p);
  return c;
}

struct DetView { double off_x, off_y; int flip_x, on; };      // on = 0: view == NULL, the box leaves as det_row returned it
struct DetCandArgs {
  int R_all, slots_per_image, classes_per_source, cand_cap, num_segs, s0, pass;
  char* cand;
  DetNms nms;
  DetSource src[kCascadeMaxOutputs];
  DetSeg seg[kSegsPerLaunch];
  DetView view[kSegsPerLaunch];
};
static_assert(sizeof(DetCandArgs) <= 4096, "DetCandArgs travels as kernel arguments");
constexpr int kCandThreads = 256;

// one workgroup per segment; steps of 256 rows, a kept row's place = the list's count + the kept rows of the waves before its own +
// those of the lower lanes of its wave (ballot / popcount, as proposals.hip).  The count is read and stored by this workgroup alone.
template <bool kThr>
__device__ __forceinline__ void det_cand_add(const DetCandArgs& a) {
  const int j = blockIdx.x, s = a.s0 + j, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int img = s / a.slots_per_image;
  const DetSource& t = a.src[(s % a.slots_per_image) / a.classes_per_source];
  const int prop_stride = t.cascade ? 5 : 6, box_stride = t.cascade ? 5 : 4 * t.ncls;
  const DetCand c = det_cand_of(a.cand, a.num_segs, a.cand_cap);
  __shared__ int s_range[2];
  __shared__ int s_base;
  __shared__ int s_cnt[kCandThreads / 64];
  if (tid < 2) s_range[tid] = det_image_lower_bound(t.props, a.R_all, img + tid, prop_stride);
  if (tid == 2) s_base = c.cnt[CAND_WORDS * (size_t)s + CAND_WANTED];
  __syncthreads();
  const int row0 = s_range[0], rows = s_range[1] - s_range[0];
  int base = s_base;
  const DetSeg& g = a.seg[j];
  DetArgs d;
  d.bbox_pred = t.boxes + (size_t)row0 * box_stride; d.cls_pred = t.cls + (size_t)row0 * t.ncls; d.props = t.props + (size_t)row0 * prop_stride;
  d.R = rows; d.ncls = t.ncls; d.cls_id = g.cls_id;
  for (int k = 0; k < 4; ++k) { d.mean[k] = g.mean[k]; d.stdv[k] = g.stdv[k]; }
  d.proposal_thr = g.proposal_thr; d.ratio_h = g.ratio_h; d.ratio_w = g.ratio_w; d.org_h = g.org_h; d.org_w = g.org_w;
  d.cascade = t.cascade;
  d.nms_thr = a.nms.thr; d.det_thr = t.cascade ? 0.f : a.nms.det_thr;
  const DetView v = a.view[j];
  const size_t list = (size_t)s * (size_t)a.cand_cap;
  for (int r0 = 0; r0 < rows; r0 += kCandThreads) {
    const int r = r0 + tid;
    DetBox b;
    float prob = 0.f;
    bool keep = false;
    if (r < rows) keep = det_row<kThr>(d, r, &b, &prob);
    const u64 m = __ballot(keep);
    if (lane == 0) s_cnt[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < kCandThreads / 64; ++w) {
      if (w < wave) before += s_cnt[w];
      total += s_cnt[w];
    }
    if (keep) {
      const long pos = (long)base + before + __popcll(m & ((1ull << lane) - 1ull));
      if (pos < (long)a.cand_cap) {                     // (past the cap nothing is stored: the count below says how many wanted in)
        if (v.on) {
          if (v.flip_x) b.x = (double)d.org_w - (b.x + b.w);
          b.x = b.x + v.off_x;
          b.y = b.y + v.off_y;
        }
        c.box[list + pos] = b;
        c.prob[list + pos] = prob;
        c.tag[list + pos] = (a.pass << 24) | (row0 + r);
      }
    }
    const long nb = (long)base + total;
    base = nb > 0x7fffffffL ? 0x7fffffff : (int)nb;
    __syncthreads();      // (every thread has read s_cnt before the next step writes it)
  }
  if (tid == 0) {
    c.cnt[CAND_WORDS * (size_t)s + CAND_WANTED] = base;
    if (base > a.cand_cap) c.cnt[CAND_WORDS * (size_t)s + CAND_OVER] = 1;
  }
}
__global__ __launch_bounds__(kCandThreads) void det_cand_add_kernel(DetCandArgs a) { det_cand_add<false>(a); }
__global__ __launch_bounds__(kCandThreads) void det_cand_add_thr_kernel(DetCandArgs a) { det_cand_add<true>(a); }

// -- the images of a batched forward into their FRAMES' lists (mscnn_detections_candidates_add_views).  A launch carries up to
// kSegsPerLaunch ENTRIES, one per (image, slot) pair, sorted by list and then by image; workgroup q owns list `list[q]` and walks its
// entries [first[q], first[q + 1]) in turn: each entry is det_cand_add's walk over that image's rows (the same det_row, view
// arithmetic, ballot / popcount places and tag) behind the count the entries before it left.  The count is read once and stored once,
// by this workgroup alone; a list whose entries do not fit one launch goes on in the next one, in stream order.
struct DetCandViewsArgs {
  int R_all, classes_per_source, cand_cap, num_segs, pass, num_blocks;      // num_segs: lists of the cand buffer
  char* cand;
  DetNms nms;
  DetSource src[kCascadeMaxOutputs];
  DetSeg seg[kSegsPerLaunch];
  DetView view[kSegsPerLaunch];
  int img[kSegsPerLaunch], slot[kSegsPerLaunch];      // entry -> its image of the batch and its slot of the image
  int list[kSegsPerLaunch], first[kSegsPerLaunch + 1];      // workgroup -> its list and its entries
};
static_assert(sizeof(DetCandViewsArgs) <= 4096, "DetCandViewsArgs travels as kernel arguments");

template <bool kThr>
__device__ __forceinline__ void det_cand_add_views(const DetCandViewsArgs& a) {
  const int q = blockIdx.x, s = a.list[q], tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const DetCand c = det_cand_of(a.cand, a.num_segs, a.cand_cap);
  __shared__ int s_range[2];
  __shared__ int s_base;
  __shared__ int s_cnt[kCandThreads / 64];
  if (tid == 0) s_base = c.cnt[CAND_WORDS * (size_t)s + CAND_WANTED];
  __syncthreads();
  int base = s_base;
  const size_t list = (size_t)s * (size_t)a.cand_cap;
  for (int e = a.first[q]; e < a.first[q + 1]; ++e) {
    const DetSource& t = a.src[a.slot[e] / a.classes_per_source];
    const int prop_stride = t.cascade ? 5 : 6, box_stride = t.cascade ? 5 : 4 * t.ncls;
    __syncthreads();      // (every thread has read the range of the entry before)
    if (tid < 2) s_range[tid] = det_image_lower_bound(t.props, a.R_all, a.img[e] + tid, prop_stride);
    __syncthreads();
    const int row0 = s_range[0], rows = s_range[1] - s_range[0];
    const DetSeg& g = a.seg[e];
    DetArgs d;
    d.bbox_pred = t.boxes + (size_t)row0 * box_stride; d.cls_pred = t.cls + (size_t)row0 * t.ncls; d.props = t.props + (size_t)row0 * prop_stride;
    d.R = rows; d.ncls = t.ncls; d.cls_id = g.cls_id;
    for (int k = 0; k < 4; ++k) { d.mean[k] = g.mean[k]; d.stdv[k] = g.stdv[k]; }
    d.proposal_thr = g.proposal_thr; d.ratio_h = g.ratio_h; d.ratio_w = g.ratio_w; d.org_h = g.org_h; d.org_w = g.org_w;
    d.cascade = t.cascade;
    d.nms_thr = a.nms.thr; d.det_thr = t.cascade ? 0.f : a.nms.det_thr;
    const DetView v = a.view[e];
    for (int r0 = 0; r0 < rows; r0 += kCandThreads) {
      const int r = r0 + tid;
      DetBox b;
      float prob = 0.f;
      bool keep = false;
      if (r < rows) keep = det_row<kThr>(d, r, &b, &prob);
      const u64 m = __ballot(keep);
      if (lane == 0) s_cnt[wave] = __popcll(m);
      __syncthreads();
      int before = 0, total = 0;
      for (int w = 0; w < kCandThreads / 64; ++w) {
        if (w < wave) before += s_cnt[w];
        total += s_cnt[w];
      }
      if (keep) {
        const long pos = (long)base + before + __popcll(m & ((1ull << lane) - 1ull));
        if (pos < (long)a.cand_cap) {                     // (past the cap nothing is stored: the count below says how many wanted in)
          if (v.on) {
            if (v.flip_x) b.x = (double)d.org_w - (b.x + b.w);
            b.x = b.x + v.off_x;
            b.y = b.y + v.off_y;
          }
          c.box[list + pos] = b;
          c.prob[list + pos] = prob;
          c.tag[list + pos] = (a.pass << 24) | (row0 + r);
        }
      }
      const long nb = (long)base + total;
      base = nb > 0x7fffffffL ? 0x7fffffff : (int)nb;
      __syncthreads();      // (every thread has read s_cnt before the next step writes it)
    }
  }
  if (tid == 0) {
    c.cnt[CAND_WORDS * (size_t)s + CAND_WANTED] = base;
    if (base > a.cand_cap) c.cnt[CAND_WORDS * (size_t)s + CAND_OVER] = 1;
  }
}
__global__ __launch_bounds__(kCandThreads) void det_cand_add_views_kernel(DetCandViewsArgs a) { det_cand_add_views<false>(a); }
__global__ __launch_bounds__(kCandThreads) void det_cand_add_views_thr_kernel(DetCandViewsArgs a) { det_cand_add_views<true>(a); }

// -- merge, lists of at most kMaxK slots: every segment in one pass, three launches per kSegsPerLaunch segments
struct DetMergeArgs {
  int cand_cap, wpr, num_segs, s0;
  char* cand; char* ws; size_t seg_stride_box, seg_stride_mask;
  int* hdr; double* dets; int* ids;
  double overlap[kSegsPerLaunch];
};
enum { MRG_N = 0, MRG_WANTED = 1, MRG_OVER = 2, MRG_WORDS = 4 };      // workspace words per segment
struct DetMergePtrs { int* cnt; DetBox* sbox; double* sprob; int* ssrc; u64* mask; };
__host__ __device__ __forceinline__ size_t det_merge_seg_box_bytes(int cap) {
  return cand_al((size_t)cap * sizeof(DetBox)) + cand_al((size_t)cap * sizeof(double)) + cand_al((size_t)cap * sizeof(int));
}
__host__ __device__ __forceinline__ size_t det_merge_seg_mask_bytes(int cap) {
  return cand_al((size_t)cap * (size_t)((cap + 63) / 64) * sizeof(u64));
}
__device__ __forceinline__ DetMergePtrs det_merge_ptrs(const DetMergeArgs& a, int s) {
  const size_t M = (size_t)a.cand_cap;
  char* base = a.ws + cand_al((size_t)a.num_segs * MRG_WORDS * sizeof(int));
  char* b = base + (size_t)s * a.seg_stride_box;
  DetMergePtrs p;
  p.cnt = reinterpret_cast<int*>(a.ws) + (size_t)s * MRG_WORDS;
  p.sbox = reinterpret_cast<DetBox*>(b);
  p.sprob = reinterpret_cast<double*>(b + cand_al(M * sizeof(DetBox)));
  p.ssrc = reinterpret_cast<int*>(b + cand_al(M * sizeof(DetBox)) + cand_al(M * sizeof(double)));
  p.mask = reinterpret_cast<u64*>(base + (size_t)a.num_segs * a.seg_stride_box + (size_t)s * a.seg_stride_mask);
  return p;
}

// one workgroup per segment: keys of the list's candidates, sort, the sorted boxes.  A list that overflowed is not run (n = 0).
__global__ __launch_bounds__(kSortThreads) void det_merge_sort_kernel(DetMergeArgs a) {
  __shared__ u64 sk[kSortCap];
  const int j = blockIdx.x, s = a.s0 + j, tid = threadIdx.x;
  const DetCand c = det_cand_of(a.cand, a.num_segs, a.cand_cap);
  const DetMergePtrs p = det_merge_ptrs(a, s);
  const int wanted = c.cnt[CAND_WORDS * (size_t)s + CAND_WANTED], over = c.cnt[CAND_WORDS * (size_t)s + CAND_OVER];
  const int n = (over || wanted > a.cand_cap) ? 0 : (wanted < 0 ? 0 : wanted);
  if (s == 0 && tid == 0) { a.hdr[0] = a.num_segs; a.hdr[1] = a.cand_cap; a.hdr[2] = a.num_segs * a.cand_cap; a.hdr[3] = 0; }
  if (tid == 0) { p.cnt[MRG_N] = n; p.cnt[MRG_WANTED] = wanted; p.cnt[MRG_OVER] = (over || wanted > a.cand_cap) ? 1 : 0; }
  if (n == 0) return;
  const size_t list = (size_t)s * (size_t)a.cand_cap;
  int P = 1;
  while (P < n) P <<= 1;
  for (int i = tid; i < P; i += kSortThreads) sk[i] = i < n ? det_key(c.prob[list + i], i) : 0ull;
  __syncthreads();
  bitonic_desc(sk, P, tid, kSortThreads);
  for (int i = tid; i < n; i += kSortThreads) {
    const int k = (int)(0xffffffffu - (unsigned)(sk[i] & 0xffffffffull));
    p.sbox[i] = c.box[list + k];
    p.sprob[i] = (double)c.prob[list + k];
    p.ssrc[i] = c.tag[list + k];
  }
}

template <bool kDnmMin>
__device__ __forceinline__ void det_merge_mask(const DetMergeArgs& a) {
  const int j = blockIdx.z, s = a.s0 + j;
  const DetMergePtrs p = det_merge_ptrs(a, s);
  det_mask_block<kDnmMin>(p.sbox, p.cnt[MRG_N], a.overlap[j], p.mask, a.wpr, blockIdx.y, blockIdx.x);
}
__global__ __launch_bounds__(256) void det_merge_mask_kernel(DetMergeArgs a) { det_merge_mask<false>(a); }
__global__ __launch_bounds__(256) void det_merge_mask_min_kernel(DetMergeArgs a) { det_merge_mask<true>(a); }

// table entry {count (-1: the list overflowed), rows that wanted in, first pack row, 0}
template <bool kGreedy>
__device__ __forceinline__ void det_merge_emit(const DetMergeArgs& a, u64* dyn_lds) {
  const int j = blockIdx.x, s = a.s0 + j;
  const DetMergePtrs p = det_merge_ptrs(a, s);
  int* ent = a.hdr + MSCNN_MULTI_PACK_WORDS * (size_t)(1 + s);
  const size_t slot = (size_t)s * (size_t)a.cand_cap;
  if (threadIdx.x == 0) { ent[1] = p.cnt[MRG_WANTED]; ent[2] = (int)slot; ent[3] = 0; }
  if (p.cnt[MRG_OVER]) { if (threadIdx.x == 0) ent[0] = -1; return; }
  if (kGreedy) det_scan_emit(p.mask, a.wpr, p.cnt[MRG_N], p.sbox, p.sprob, p.ssrc, a.dets + 5 * slot, a.ids + slot, ent, dyn_lds);
  else det_color_emit(p.mask, a.wpr, p.cnt[MRG_N], p.sbox, p.sprob, p.ssrc, a.dets + 5 * slot, a.ids + slot, ent, dyn_lds);
}
__global__ __launch_bounds__(256) void det_merge_scan_emit_kernel(DetMergeArgs a) {
  extern __shared__ __attribute__((aligned(16))) u64 dyn_lds[];
  det_merge_emit<true>(a, dyn_lds);
}
__global__ __launch_bounds__(256) void det_merge_color_emit_kernel(DetMergeArgs a) {
  extern __shared__ __attribute__((aligned(16))) u64 dyn_lds[];
  det_merge_emit<false>(a, dyn_lds);
}

// -- merge, lists of more than kMaxK slots: one list at a time on the tiled kernels (nms_large.h)
// keys[0 .. P): the list's keys, then zero padding; cnt[DC_N] = the list's length (0 when it overflowed), the tiled path's state cleared
__global__ __launch_bounds__(256) void det_merge_keys_big_kernel(const int* __restrict__ lcnt, const float* __restrict__ prob, int cap,
                                                                 u64* __restrict__ keys, int P, int* __restrict__ cnt) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int wanted = lcnt[CAND_WANTED];
  const int n = (lcnt[CAND_OVER] || wanted > cap || wanted < 0) ? 0 : wanted;
  if (i == 0) { cnt[DC_N] = n; cnt[DC_BIG + BIG_TILE_N] = 0; cnt[DC_BIG + BIG_NKEPT] = 0; }
  if (i < P) keys[i] = i < n ? det_key(prob[i], i) : 0ull;
}
__global__ __launch_bounds__(256) void det_merge_gather_big_kernel(const u64* __restrict__ keys, const DetBox* __restrict__ box,
                                                                   const float* __restrict__ prob, const int* __restrict__ tag,
                                                                   DetBox* __restrict__ sbox, double* __restrict__ sprob,
                                                                   int* __restrict__ ssrc, const int* __restrict__ cnt) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= cnt[DC_N]) return;
  const int k = (int)(0xffffffffu - (unsigned)(keys[i] & 0xffffffffull));
  sbox[i] = box[k];
  sprob[i] = (double)prob[k];
  ssrc[i] = tag[k];
}
// header and the table words the emit kernel does not write; runs behind the last list's emit (which stored every count)
__global__ __launch_bounds__(256) void det_merge_table_big_kernel(const int* __restrict__ lcnt, int S, int cap, int* __restrict__ hdr) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s == 0) { hdr[0] = S; hdr[1] = cap; hdr[2] = S * cap; hdr[3] = 0; }
  if (s >= S) return;
  const int wanted = lcnt[CAND_WORDS * (size_t)s + CAND_WANTED];
  int* ent = hdr + MSCNN_MULTI_PACK_WORDS * (size_t)(1 + s);
  if (lcnt[CAND_WORDS * (size_t)s + CAND_OVER] || wanted > cap) ent[0] = -1;
  ent[1] = wanted; ent[2] = s * cap; ent[3] = 0;
}

// -- box voting behind the merge (mscnn_detections_merge_vote_fwd): every kept row of the pack becomes the prob-weighted mean of the
// list's candidates that overlap it.  One wave64 per kept row, the kVoteRows waves of a workgroup share the tile of kVoteThreads
// candidates they stream through LDS.  SUMMATION ORDER (mscnn_hip.h): lane l adds the voters among slots l, l + 64, ... in ascending
// order, then an xor butterfly over 32, 16, ..., 1 -- IEEE addition commutes, so both lanes of a pair get the same bits and no lane
// has to broadcast.  The order is a function of the slot index alone: which workgroup takes a row (the groups of four rows of all
// segments, counted through, go round the fixed grid) decides nothing about it.  A row reads the candidates and itself, and is
// written by its own wave: in place is safe.  No atomics, no workgroup waits on another.
constexpr int kVoteThreads = 256, kVoteRows = kVoteThreads / 64, kVoteBlocks = 256;
struct DetVoteArgs { int num_segs, cand_cap; double thr; char* cand; const int* hdr; double* dets; };

__global__ __launch_bounds__(kVoteThreads) void det_merge_vote_kernel(DetVoteArgs a) {
  __shared__ DetBox tbox[kVoteThreads];
  __shared__ float tprob[kVoteThreads];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grid = (int)gridDim.x;
  const DetCand c = det_cand_of(a.cand, a.num_segs, a.cand_cap);      // (read only)
  int first = (int)blockIdx.x;      // this workgroup's first group of the segment at hand: the groups of all segments go round the grid
  for (int s = 0; s < a.num_segs; ++s) {
    // (every value that bounds a loop or guards a barrier below is the same in all threads of the workgroup)
    const int D = min(a.hdr[MSCNN_MULTI_PACK_WORDS * (size_t)(1 + s)], a.cand_cap);      // -1: the list overflowed, nothing of it is touched
    if (D <= 0) continue;
    const int wanted = c.cnt[CAND_WORDS * (size_t)s + CAND_WANTED];
    const int n = wanted < 0 ? 0 : min(wanted, a.cand_cap);
    const int groups = (D + kVoteRows - 1) / kVoteRows;
    const size_t list = (size_t)s * (size_t)a.cand_cap;
    int g = first;
    first = (int)(((long)first + grid - groups % grid) % grid);
    for (; g < groups; g += grid) {
      const int k = g * kVoteRows + wave;
      const bool live = k < D;
      double* row = a.dets + 5 * (list + (size_t)(live ? k : 0));
      DetBox A = DetBox{0.0, 0.0, 0.0, 0.0};
      if (live) A = DetBox{row[0], row[1], row[2], row[3]};
      const double as_a = A.w * A.h, xe_a = A.x + A.w, ye_a = A.y + A.h;
      double sp = 0.0, sx = 0.0, sy = 0.0, sw = 0.0, sh = 0.0;
      int voters = 0;
      for (int t0 = 0; t0 < n; t0 += kVoteThreads) {
        __syncthreads();      // (every wave is done with the tile before)
        if (t0 + tid < n) { tbox[tid] = c.box[list + t0 + tid]; tprob[tid] = c.prob[list + t0 + tid]; }
        __syncthreads();
        if (!live) continue;
        const int tn = min(kVoteThreads, n - t0);
        for (int q = lane; q < tn; q += 64) {
          const DetBox B = tbox[q];
          const double iw = fmin(xe_a, B.x + B.w) - fmax(A.x, B.x);      // DetTr::over / det_mask_block, the union form
          if (iw <= 0) continue;
          const double ih = fmin(ye_a, B.y + B.h) - fmax(A.y, B.y);
          if (ih <= 0) continue;
          double o = iw * ih;
          const double u = as_a + B.w * B.h - o;
          o = o / u;
          if (!(o >= a.thr)) continue;      // (a NaN ratio does not vote)
          const double p = (double)tprob[q];
          sp = sp + p;
          sx = sx + p * B.x; sy = sy + p * B.y; sw = sw + p * B.w; sh = sh + p * B.h;
          ++voters;
        }
      }
      for (int m = 32; m >= 1; m >>= 1) {
        sp = sp + __shfl_xor(sp, m); sx = sx + __shfl_xor(sx, m); sy = sy + __shfl_xor(sy, m);
        sw = sw + __shfl_xor(sw, m); sh = sh + __shfl_xor(sh, m);
        voters += __shfl_xor(voters, m);
      }
      // fewer than two voters (the row itself, as a rule), or weights that do not sum above zero: the row stays bit for bit
      if (live && lane == 0 && voters >= 2 && sp > 0) { row[0] = sx / sp; row[1] = sy / sp; row[2] = sw / sp; row[3] = sh / sp; }
    }
  }
}

// -- Soft-NMS over the merged candidates (mscnn_detections_merge_soft_fwd): serial in picks, parallel in candidates.  One workgroup of
// kSoftThreads owns a list; thread t owns slots t, t + kSoftThreads, ... for the whole call, so a score or a live flag is only ever
// read and written by its own thread.  A pick: every thread's best live candidate, a reduction over the wave's 64 lanes (DPP row
// rotations inside the rows of 16, an xor butterfly across them), the wave's winner -- score, slot and box, written by its owner --
// into one of two LDS buffers, ONE barrier, then every wave reduces the kSoftWaves entries (one per lane of a row), finds the same
// winner, and every thread decays its own candidates by that box while it looks for its next best.  The buffers alternate: a
// thread writes buffer k & 1 for pick k + 2 only behind barrier k + 1, which every thread reaches behind its reads of pick k.
// The winner is a maximum under a total order (soft_better: score, then the lower slot): nothing depends on the shape of
// the reduction.  A list of at most kSoftRegs candidates lives in registers (box, score, tag and live bit of kSoftPer slots per
// thread); a longer one keeps scores and live flags in the workspace and reads boxes and tags from the candidate buffer -- the same
// soft_decay per candidate, the same bits.  Every loop bound and every value that guards the barrier is a kernel argument, the
// list's device count or the winner read out of LDS as a scalar, the same in all threads; a pick kills one candidate, so the loop runs at most n times; no atomics, nothing spins,
// no workgroup waits on another.
constexpr int kSoftThreads = 1024, kSoftWaves = kSoftThreads / 64, kSoftPer = 4, kSoftRegs = kSoftThreads * kSoftPer;
constexpr int kSoftNone = 0x7fffffff;      // the slot of "nothing live": loses every tie
struct DetSoftArgs {
  int cand_cap, num_segs, s0, method, max_out;
  double sigma, score_thr;
  char* cand; char* ws; size_t seg_stride;
  int* hdr; double* dets; int* ids;
  double overlap[kSegsPerLaunch];
};
struct SoftBest { double s; int slot; };
struct SoftPick { double s; int slot; int pad; DetBox box; };

__host__ __device__ __forceinline__ size_t det_soft_seg_bytes(int cap) {      // the streaming path's scores and live flags of one list
  return cap > kSoftRegs ? cand_al((size_t)cap * sizeof(double)) + cand_al((size_t)cap) : 0;
}
// a NaN ranks below every number
__device__ __forceinline__ double soft_rank(double s) { return s != s ? -__builtin_inf() : s; }
// the total order of the argmax: the larger score, then the lower slot
__device__ __forceinline__ bool soft_better(double sa, int ia, double sb, int ib) { return sa > sb || (sa == sb && ia < ib); }
__device__ __forceinline__ void soft_take(SoftBest& b, double s, int slot) {
  s = soft_rank(s);
  if (soft_better(s, slot, b.s, b.slot)) { b.s = s; b.slot = slot; }
}
// the score of candidate B after the pick of box A (step 5 of the contract, one statement per operation: the vote's overlap)
struct SoftDecay { DetBox A; double as_a, xe_a, ye_a, overlap, sigma; bool linear; };
__device__ __forceinline__ SoftDecay soft_decay_of(const DetBox& A, double overlap, double sigma, int method) {
  return SoftDecay{A, A.w * A.h, A.x + A.w, A.y + A.h, overlap, sigma, method == MSCNN_SOFT_NMS_LINEAR};
}
__device__ __forceinline__ double soft_decay(const SoftDecay& d, const DetBox& B, double s) {
  const double iw = fmin(d.xe_a, B.x + B.w) - fmax(d.A.x, B.x);
  if (iw <= 0) return s;
  const double ih = fmin(d.ye_a, B.y + B.h) - fmax(d.A.y, B.y);
  if (ih <= 0) return s;
  const double o = iw * ih;
  const double u = d.as_a + B.w * B.h - o;
  const double r = o / u;
  if (r != r) return s;
  if (d.linear) return r > d.overlap ? s * (1.0 - r) : s;
  return s * exp(-(r * r) / d.sigma);
}
// lane i of a row of 16 lanes <- lane i - n (mod 16) of that row: a DPP row rotation, no LDS traffic; every lane has a source
template <int kRor> __device__ __forceinline__ int soft_ror(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x120 + kRor, 0xf, 0xf, false); }
template <int kRor> __device__ __forceinline__ void soft_row_step(SoftBest& b) {
  const double so = __hiloint2double(soft_ror<kRor>(__double2hiint(b.s)), soft_ror<kRor>(__double2loint(b.s)));
  const int io = soft_ror<kRor>(b.slot);
  if (soft_better(so, io, b.s, b.slot)) { b.s = so; b.slot = io; }
}
// the best of every row of 16 lanes into all 16: rotations by 1, 2, 4 and 8 cover the row (a maximum under a total order is
// idempotent: a candidate met twice changes nothing, so the shape of the reduction is free)
__device__ __forceinline__ SoftBest soft_row_best(SoftBest b) {
  soft_row_step<1>(b); soft_row_step<2>(b); soft_row_step<4>(b); soft_row_step<8>(b);
  return b;
}
// the wave's best into every lane: the four rows, then an xor butterfly over 16 and 32
__device__ __forceinline__ SoftBest soft_wave_best(SoftBest b) {
  b = soft_row_best(b);
  for (int m = 16; m <= 32; m <<= 1) {
    const double so = __shfl_xor(b.s, m);
    const int io = __shfl_xor(b.slot, m);
    if (soft_better(so, io, b.s, b.slot)) { b.s = so; b.slot = io; }
  }
  return b;
}
// the workgroup's winner out of the kSoftWaves entries: lane l reads entry l mod 16, so every row holds them all and reduces them;
// the result is the same in every lane and leaves as a scalar -- what guards the barrier is uniform for the compiler too
static_assert(kSoftWaves == 16, "soft_winner: one entry per lane of a DPP row");
__device__ __forceinline__ SoftBest soft_winner(const SoftPick* buf, int tid) {
  const SoftPick& e = buf[tid & (kSoftWaves - 1)];
  const SoftBest b = soft_row_best(SoftBest{e.s, e.slot});
  return SoftBest{__hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(b.s)), __builtin_amdgcn_readfirstlane(__double2loint(b.s))),
                  __builtin_amdgcn_readfirstlane(b.slot)};
}
// the entry of `buf` that holds slot m: its owner's wave wrote it
__device__ __forceinline__ int soft_entry_of(int m) { return (m & (kSoftThreads - 1)) >> 6; }

__global__ __launch_bounds__(kSoftThreads) void det_merge_soft_kernel(DetSoftArgs a) {
  __shared__ SoftPick pick[2][kSoftWaves];
  const int j = blockIdx.x, s = a.s0 + j, tid = threadIdx.x, wave = tid >> 6;
  const DetCand c = det_cand_of(a.cand, a.num_segs, a.cand_cap);      // (read only)
  const int wanted = c.cnt[CAND_WORDS * (size_t)s + CAND_WANTED], over = c.cnt[CAND_WORDS * (size_t)s + CAND_OVER];
  const size_t list = (size_t)s * (size_t)a.cand_cap;
  int* ent = a.hdr + MSCNN_MULTI_PACK_WORDS * (size_t)(1 + s);
  if (s == 0 && tid == 0) { a.hdr[0] = a.num_segs; a.hdr[1] = a.cand_cap; a.hdr[2] = a.num_segs * a.cand_cap; a.hdr[3] = 0; }
  if (tid == 0) { ent[1] = wanted; ent[2] = (int)list; ent[3] = 0; }
  if (over || wanted > a.cand_cap) { if (tid == 0) ent[0] = -1; return; }      // the list overflowed: nothing else of it is written
  const int n = wanted < 0 ? 0 : wanted;
  const DetBox* box = c.box + list;
  const float* prob = c.prob + list;
  const int* tag = c.tag + list;
  double* dets = a.dets + 5 * list;
  int* ids = a.ids + list;
  const double overlap = a.overlap[j];
  const int max_out = a.max_out > 0 ? a.max_out : n;      // (a pick kills a candidate: n picks at the most)
  int D = 0;

  if (n <= kSoftRegs) {
    // ---- the list in registers: slot tid + q * kSoftThreads is this thread's q-th
    DetBox rb[kSoftPer];
    double rs[kSoftPer];
    int rt[kSoftPer];
    unsigned live = 0;
    SoftBest best = {-__builtin_inf(), kSoftNone};
#pragma unroll
    for (int q = 0; q < kSoftPer; ++q) {
      const int i = tid + q * kSoftThreads;
      rb[q] = DetBox{0.0, 0.0, 0.0, 0.0}; rs[q] = 0.0; rt[q] = 0;
      if (i < n) {
        rb[q] = box[i]; rs[q] = (double)prob[i]; rt[q] = tag[i];
        live |= 1u << q;
        soft_take(best, rs[q], i);
      }
    }
    for (; D < max_out; ++D) {
      SoftPick* buf = pick[D & 1];
      best = soft_wave_best(best);
      if (best.slot != kSoftNone && (best.slot & (kSoftThreads - 1)) == tid) {      // this thread owns the wave's winner
        const int q = best.slot / kSoftThreads;
        DetBox B = rb[0];
#pragma unroll
        for (int k = 1; k < kSoftPer; ++k) if (q == k) B = rb[k];
        buf[wave].s = best.s; buf[wave].slot = best.slot; buf[wave].box = B;
      } else if ((tid & 63) == 0 && best.slot == kSoftNone) {
        buf[wave].s = best.s; buf[wave].slot = kSoftNone;
      }
      __syncthreads();
      const SoftBest W = soft_winner(buf, tid);
      const int m = W.slot;
      if (m == kSoftNone || !(W.s >= a.score_thr)) break;      // nothing live, or the best is under the threshold (a NaN included)
      const SoftDecay d = soft_decay_of(buf[soft_entry_of(m)].box, overlap, a.sigma, a.method);
      if ((m & (kSoftThreads - 1)) == tid) {      // the owner emits the row and retires the candidate
        const int q = m / kSoftThreads;
        int t = rt[0];
#pragma unroll
        for (int k = 1; k < kSoftPer; ++k) if (q == k) t = rt[k];
        dets[5 * (size_t)D + 0] = d.A.x; dets[5 * (size_t)D + 1] = d.A.y; dets[5 * (size_t)D + 2] = d.A.w; dets[5 * (size_t)D + 3] = d.A.h;
        dets[5 * (size_t)D + 4] = W.s;
        ids[D] = t;
        live &= ~(1u << q);
      }
      best = SoftBest{-__builtin_inf(), kSoftNone};
#pragma unroll
      for (int q = 0; q < kSoftPer; ++q) {
        if (live & (1u << q)) {
          rs[q] = soft_decay(d, rb[q], rs[q]);
          soft_take(best, rs[q], tid + q * kSoftThreads);
        }
      }
    }
  } else {
    // ---- the list streamed: scores and live flags in the workspace (this thread's slots only), boxes from the candidate buffer
    char* w = a.ws + (size_t)j * a.seg_stride;
    double* ws_s = reinterpret_cast<double*>(w);
    unsigned char* ws_live = reinterpret_cast<unsigned char*>(w + cand_al((size_t)a.cand_cap * sizeof(double)));
    SoftBest best = {-__builtin_inf(), kSoftNone};
    for (int i = tid; i < n; i += kSoftThreads) {
      const double v = (double)prob[i];
      ws_s[i] = v; ws_live[i] = 1;
      soft_take(best, v, i);
    }
    for (; D < max_out; ++D) {
      SoftPick* buf = pick[D & 1];
      best = soft_wave_best(best);
      if (best.slot != kSoftNone && (best.slot & (kSoftThreads - 1)) == tid) {
        buf[wave].s = best.s; buf[wave].slot = best.slot; buf[wave].box = box[best.slot];
      } else if ((tid & 63) == 0 && best.slot == kSoftNone) {
        buf[wave].s = best.s; buf[wave].slot = kSoftNone;
      }
      __syncthreads();
      const SoftBest W = soft_winner(buf, tid);
      const int m = W.slot;
      if (m == kSoftNone || !(W.s >= a.score_thr)) break;
      const SoftDecay d = soft_decay_of(buf[soft_entry_of(m)].box, overlap, a.sigma, a.method);
      if ((m & (kSoftThreads - 1)) == tid) {
        dets[5 * (size_t)D + 0] = d.A.x; dets[5 * (size_t)D + 1] = d.A.y; dets[5 * (size_t)D + 2] = d.A.w; dets[5 * (size_t)D + 3] = d.A.h;
        dets[5 * (size_t)D + 4] = W.s;
        ids[D] = tag[m];
        ws_live[m] = 0;
      }
      best = SoftBest{-__builtin_inf(), kSoftNone};
      for (int i = tid; i < n; i += kSoftThreads) {
        if (!ws_live[i]) continue;
        const double v = soft_decay(d, box[i], ws_s[i]);
        ws_s[i] = v;
        soft_take(best, v, i);
      }
    }
  }
  if (tid == 0) ent[0] = D;      // (D is the same in every thread)
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
struct DetLayout { size_t cnt, sbox, sprob, ssrc, tbox, tprob, mask, keys, rinit, kidx, kbox, total; int wpr, sortP; bool big; };
DetLayout det_layout(int R) {
  DetLayout L;
  const int n = R < 1 ? 1 : R;
  L.big = n > kMaxK;                         // more rows than the LDS-resident path holds: sort in HBM, tiled NMS
  L.wpr = L.big ? kTileWords : (n + 63) / 64;
  L.sortP = L.big ? big_sort_pow2(n) : 0;
  size_t o = 0;
  L.cnt = o; o += 256;                       // [DC_N ...] and, at DC_BIG, the tiled path's state words
  L.sbox = o; o += align_up((size_t)n * sizeof(DetBox), 256);
  L.sprob = o; o += align_up((size_t)n * sizeof(double), 256);
  L.ssrc = o; o += align_up((size_t)n * sizeof(int), 256);
  L.tbox = o; o += align_up((size_t)n * sizeof(DetBox), 256);
  L.tprob = o; o += align_up((size_t)n * sizeof(float), 256);
  L.mask = o; o += align_up((size_t)(L.big ? kMaxK : n) * L.wpr * sizeof(u64), 256);
  L.keys = o; o += L.big ? align_up((size_t)L.sortP * sizeof(u64), 256) : 0;
  L.rinit = o; o += L.big ? align_up(64 * sizeof(u64), 256) : 0;
  L.kidx = o; o += L.big ? align_up((size_t)n * sizeof(int), 256) : 0;
  L.kbox = o; o += L.big ? align_up((size_t)n * sizeof(DetBox), 256) : 0;
  L.total = o;
  return L;
}
}  // namespace

using namespace mscnn;

extern "C" int mscnn_decodebbox_fwd_f32(const float* bbox, const float* prior, float* out, int R, int bbox_dim,
                                        const float* mean_host, const float* std_host, void* stream) {
  MSCNN_REQUIRE(R >= 0, "decodebbox: R < 0");
  MSCNN_REQUIRE(bbox_dim == 8, "decodebbox: bbox channels must be 8 (decode_bbox_layer.cpp:47), got %d", bbox_dim);
  if (R == 0) return MSCNN_OK;
  MSCNN_REQUIRE(bbox && prior && out && mean_host && std_host, "decodebbox: null pointer");
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
static bool nms_has_thr(const mscnn_nms_params& r) { return r.thr != -HUGE_VAL || r.det_thr != 0.f; }
static DetNms det_nms_of(const mscnn_nms_params& r) { return DetNms{r.thr, r.det_thr, r.type, r.ovr_dnm}; }

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
    u64* keys = reinterpret_cast<u64*>(ws + L.keys);
    int* kidx = reinterpret_cast<int*>(ws + L.kidx);
    MSCNN_HIP_TRY(hipMemsetAsync(cnt, 0, 256, st));
    MSCNN_HIP_TRY(hipMemsetAsync(keys, 0, (size_t)L.sortP * sizeof(u64), st));
    det_transform_big_kernel<<<cdiv(R, 256), 256, 0, st>>>(a, keys, tbox, tprob, cnt);
    MSCNN_POST_LAUNCH();
    MSCNN_HIP_TRY(big_sort_desc(keys, L.sortP, st));
    det_gather_big_kernel<<<cdiv(R, 256), 256, 0, st>>>(keys, tbox, tprob, sbox, sprob, ssrc, cnt);
    MSCNN_POST_LAUNCH();
    const double overlap = desc->nms_overlap;
    auto launch_mask = [&](const DetBox* tile, const int* tile_n) {
      det_mask_kernel<<<dim3(kTileWords, kTileWords), 256, 0, st>>>(tile, tile_n, overlap, mask, kTileWords);
    };
    MSCNN_HIP_TRY((big_nms_tiles<DetTr>(sbox, cnt + DC_N, 0, R, DetTr::Params{overlap}, mask, reinterpret_cast<u64*>(ws + L.rinit), kidx,
                                        reinterpret_cast<DetBox*>(ws + L.kbox), cnt + DC_BIG, launch_mask, st)));
    det_emit_big_kernel<<<cdiv(R, 256), 256, 0, st>>>(kidx, cnt + DC_BIG, sbox, sprob, ssrc, dets_out, ids_out, count_out_dev);
    MSCNN_POST_LAUNCH();
    return MSCNN_OK;
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
static size_t det_multi_seg_box_bytes(int M) {
  const size_t m = (size_t)(M < 1 ? 1 : M);
  return 2 * align_up(m * sizeof(DetBox), 256) + align_up(m * sizeof(double), 256) + align_up(m * sizeof(int), 256) +
         align_up(m * sizeof(float), 256);
}
static size_t det_multi_seg_mask_bytes(int M) {
  const size_t m = (size_t)(M < 1 ? 1 : M);
  return align_up(m * (size_t)((m + 63) / 64) * sizeof(u64), 256);
}

extern "C" size_t mscnn_detections_multi_pack_bytes(int num_segments, int cap) {
  return mscnn_multi_pack_layout_of(num_segments, cap).total;
}

extern "C" size_t mscnn_detections_multi_workspace_bytes(int num_segments, int max_rows_per_image) {
  if (num_segments < 1 || max_rows_per_image > kMaxK) return 0;
  const int M = max_rows_per_image < 1 ? 1 : max_rows_per_image;
  return align_up((size_t)num_segments * SEG_WORDS * sizeof(int), 256) +
         (size_t)num_segments * (det_multi_seg_box_bytes(M) + det_multi_seg_mask_bytes(M));
}
extern "C" size_t mscnn_detections_cascade_multi_workspace_bytes(int num_segments, int max_rows_per_image) {
  return mscnn_detections_multi_workspace_bytes(num_segments, max_rows_per_image);
}

// cascade: proposal_thr = det_thr (run_cascademscnn.m:115-117), mean 0 / std 1 (not read by the cascade row transform)
static DetSeg det_seg_of(const mscnn_detections_desc& d, int cascade, float det_thr) {
  DetSeg g;
  for (int k = 0; k < 4; ++k) { g.mean[k] = cascade ? 0.f : d.bbox_mean[k]; g.stdv[k] = cascade ? 1.f : d.bbox_std[k]; }
  g.proposal_thr = cascade ? det_thr : d.proposal_thr; g.cls_id = d.cls_id; g.nms_overlap = d.nms_overlap;
  // MATLAB: single op double -> single (as detections_launch)
  g.ratio_h = (float)d.ratio_h; g.ratio_w = (float)d.ratio_w; g.org_h = (float)d.org_h; g.org_w = (float)d.org_w;
  return g;
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
  a.seg_stride_box = det_multi_seg_box_bytes(M); a.seg_stride_mask = det_multi_seg_mask_bytes(M);
  for (int o = 0; o < num_sources; ++o) a.src[o] = src[o];
  const mscnn_multi_pack_layout L = mscnn_multi_pack_layout_of(S, cap);
  char* pk = static_cast<char*>(pack_dev);
  a.hdr = reinterpret_cast<int*>(pk);
  a.dets = reinterpret_cast<double*>(pk + L.dets);
  a.ids = reinterpret_cast<int*>(pk + L.ids);
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
  const int ncls = desc[0].ncls;
  for (int s = 0; s < S; ++s)
    MSCNN_REQUIRE(desc[s].ncls == ncls && desc[s].cls_id >= 1 && desc[s].cls_id <= ncls && ncls >= 2,
                  "detections_multi: segment %d: cls_id %d of %d", s, desc[s].cls_id, desc[s].ncls);
  const size_t need = mscnn_detections_multi_workspace_bytes(S, max_rows_per_image);
  if (workspace_bytes < need) {
    set_error("detections_multi: workspace %zu < %zu", workspace_bytes, need);
    return MSCNN_ERR_WORKSPACE;
  }
  const DetSource src = {bbox_pred, cls_pred, props, ncls, 0};
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
  mscnn_nms_params nms;
  if (int rc = mscnn_nms_params_resolve(nms_in, &nms)) return rc;
  MSCNN_REQUIRE(nms.det_thr == 0.f, "detections_cascade_multi: nms params det_thr %g is the plain stage's: the cascade stage takes its "
                "det_thr as an argument", (double)nms.det_thr);
  MSCNN_REQUIRE(num_outputs >= 1 && num_outputs <= kCascadeMaxOutputs, "detections_cascade_multi: %d cascade outputs (1 .. %d)",
                num_outputs, kCascadeMaxOutputs);
  MSCNN_REQUIRE(desc && outputs && pack_dev && workspace, "detections_cascade_multi: null pointer");
  MSCNN_REQUIRE_ALIGNED(pack_dev, 16, "detections_cascade_multi: pack_dev");
  MSCNN_REQUIRE_ALIGNED(workspace, 16, "detections_cascade_multi: workspace");
  MSCNN_REQUIRE(num_images >= 1 && num_classes >= 1, "detections_cascade_multi: %d images x %d classes", num_images, num_classes);
  MSCNN_REQUIRE(R_all >= 1, "detections_cascade_multi: R_all = %d (BoxOutput emits at least one row)", R_all);
  for (int o = 0; o < num_outputs; ++o) {
    MSCNN_REQUIRE(outputs[o].boxes && outputs[o].cls_prob && outputs[o].props, "detections_cascade_multi: output %d of %d: null pointer",
                  o, num_outputs);
    MSCNN_REQUIRE(outputs[o].ncls >= 2, "detections_cascade_multi: output %d: %d probability columns", o, outputs[o].ncls);
  }
  MSCNN_REQUIRE(max_rows_per_image >= 1 && max_rows_per_image <= kMaxK,
                "detections_cascade_multi: %d rows per image > %d: run mscnn_detections_cascade_fwd per segment", max_rows_per_image, kMaxK);
  const int K = num_outputs * num_classes;
  MSCNN_REQUIRE((long)K * R_all <= (long)cap, "detections_cascade_multi: pack capacity %d < %d outputs x %d classes x %d ROIs", cap,
                num_outputs, num_classes, R_all);
  MSCNN_REQUIRE((long)num_images * K <= (long)(1 << 24), "detections_cascade_multi: %d images x %d outputs x %d classes", num_images,
                num_outputs, num_classes);
  const int S = num_images * K;
  for (int s = 0; s < S; ++s) {
    const int o = (s % K) / num_classes;
    MSCNN_REQUIRE(desc[s].cls_id >= 1 && desc[s].cls_id <= outputs[o].ncls, "detections_cascade_multi: segment %d (output %d): cls_id %d of %d",
                  s, o, desc[s].cls_id, outputs[o].ncls);
  }
  const size_t need = mscnn_detections_cascade_multi_workspace_bytes(S, max_rows_per_image);
  if (workspace_bytes < need) {
    set_error("detections_cascade_multi: workspace %zu < %zu", workspace_bytes, need);
    return MSCNN_ERR_WORKSPACE;
  }
  DetSource src[kCascadeMaxOutputs];
  for (int o = 0; o < num_outputs; ++o) src[o] = DetSource{outputs[o].boxes, outputs[o].cls_prob, outputs[o].props, outputs[o].ncls, 1};
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

// ---- candidate lists of several forwards, one NMS over each (mscnn_hip.h) -------------------------------------------------------------
static bool cand_shape_ok(int S, int cand_cap) { return S >= 1 && cand_cap >= 1 && (long)S * (long)cand_cap <= 0x7fffffffL; }

extern "C" size_t mscnn_detections_candidates_bytes(int num_segments, int cand_cap) {
  return cand_shape_ok(num_segments, cand_cap) ? det_cand_bytes(num_segments, cand_cap) : 0;
}

extern "C" int mscnn_detections_candidates_reset(void* cand, int num_segments, int cand_cap, void* stream) {
  MSCNN_REQUIRE(cand, "detections_candidates_reset: null pointer");
  MSCNN_REQUIRE(num_segments >= 1, "detections_candidates_reset: %d segments", num_segments);
  MSCNN_REQUIRE(cand_cap >= 1, "detections_candidates_reset: cand_cap %d", cand_cap);
  MSCNN_REQUIRE(cand_shape_ok(num_segments, cand_cap), "detections_candidates_reset: %d segments x %d slots is past 2^31 - 1", num_segments,
                cand_cap);
  MSCNN_REQUIRE_ALIGNED(cand, 16, "detections_candidates_reset: cand");
  MSCNN_HIP_TRY(hipMemsetAsync(cand, 0, (size_t)num_segments * CAND_WORDS * sizeof(int), as_stream(stream)));
  return MSCNN_OK;
}

// the views form: entries (image, slot) sorted by list and then by image, 32 per launch, one workgroup per list of a launch
static int det_cand_views_launch(const DetSource* src, int num_sources, const mscnn_detections_desc* desc, const mscnn_detections_view* view,
                                 const int* list_of, float det_thr, const mscnn_nms_params& nms, int pass, int num_images, int num_lists,
                                 int C, int R_all, void* cand, int cand_cap, hipStream_t st) {
  const int K = num_sources * C;
  DetCandViewsArgs a = {};
  a.R_all = R_all; a.classes_per_source = C; a.cand_cap = cand_cap; a.num_segs = num_lists * K; a.pass = pass;
  a.cand = static_cast<char*>(cand);
  a.nms = det_nms_of(nms);
  for (int o = 0; o < num_sources; ++o) a.src[o] = src[o];
  // (list-major, then the image index ascending: per frame its images in turn, each with its K slots)
  std::vector<std::vector<int> > images_of(num_lists);
  for (int b = 0; b < num_images; ++b) images_of[list_of[b]].push_back(b);
  int n = 0, last_list = -1;
  auto flush = [&]() -> int {
    if (n == 0) return MSCNN_OK;
    a.first[a.num_blocks] = n;
    if (nms_has_thr(nms)) det_cand_add_views_thr_kernel<<<a.num_blocks, kCandThreads, 0, st>>>(a);
    else det_cand_add_views_kernel<<<a.num_blocks, kCandThreads, 0, st>>>(a);
    MSCNN_POST_LAUNCH();
    n = 0; a.num_blocks = 0; last_list = -1;
    return MSCNN_OK;
  };
  for (int f = 0; f < num_lists; ++f) {
    for (int k = 0; k < K; ++k) {
      for (int b : images_of[f]) {
        const int s = f * K + k;
        if (s != last_list) { a.list[a.num_blocks] = s; a.first[a.num_blocks] = n; ++a.num_blocks; last_list = s; }
        a.seg[n] = det_seg_of(desc[b * K + k], src[0].cascade, det_thr);
        a.view[n] = view ? DetView{view[b].off_x, view[b].off_y, view[b].flip_x, 1} : DetView{0.0, 0.0, 0, 0};
        a.img[n] = b; a.slot[n] = k;
        if (++n == kSegsPerLaunch) { if (int rc = flush()) return rc; }
      }
    }
  }
  return flush();
}

// everything the add calls refuse alike, then one launch per 32 segments.  list_of != NULL: the views form (S lists = num_lists x K)
static int det_cand_launch(const char* name, const DetSource* src, int num_sources, const mscnn_detections_desc* desc,
                           const mscnn_detections_view* view, float det_thr, const mscnn_nms_params& nms, int pass, int num_images, int C,
                           int R_all, void* cand, int cand_cap, void* stream, const int* list_of = nullptr, int num_lists = 0) {
  const int K = num_sources * C;
  MSCNN_REQUIRE((long)num_images * K <= (long)(1 << 24), "%s: %d images x %d slots", name, num_images, K);
  MSCNN_REQUIRE(!list_of || (long)num_lists * K <= (long)(1 << 24), "%s: %d lists x %d slots", name, num_lists, K);
  const int S = (list_of ? num_lists : num_images) * K;
  MSCNN_REQUIRE(cand_cap >= 1, "%s: cand_cap %d", name, cand_cap);
  MSCNN_REQUIRE(cand_shape_ok(S, cand_cap), "%s: %d segments x %d slots is past 2^31 - 1", name, S, cand_cap);
  MSCNN_REQUIRE_ALIGNED(cand, 16, "detections_candidates: cand");
  MSCNN_REQUIRE(pass >= 0 && pass <= 127, "%s: pass %d (0 .. 127: the tag is (pass << 24) | row)", name, pass);
  MSCNN_REQUIRE(R_all >= 1, "%s: R_all = %d (BoxOutput emits at least one row)", name, R_all);
  MSCNN_REQUIRE(R_all < (1 << 24), "%s: R_all = %d rows do not fit the tag's 24 row bits", name, R_all);
  for (int s = 0; s < num_images * K; ++s) {
    MSCNN_REQUIRE(desc[s].ratio_h > 0 && desc[s].ratio_w > 0, "%s: segment %d: ratios %g x %g (positive numbers)", name, s, desc[s].ratio_h,
                  desc[s].ratio_w);
  }
  for (int i = 0; view && i < num_images; ++i) {
    MSCNN_REQUIRE(std::isfinite(view[i].off_x) && std::isfinite(view[i].off_y), "%s: image %d: view offset (%g, %g) is not finite", name, i,
                  view[i].off_x, view[i].off_y);
    MSCNN_REQUIRE(view[i].flip_x == 0 || view[i].flip_x == 1, "%s: image %d: flip_x %d (0 or 1)", name, i, view[i].flip_x);
  }
  hipStream_t st = as_stream(stream);
  if (list_of)
    return det_cand_views_launch(src, num_sources, desc, view, list_of, det_thr, nms, pass, num_images, num_lists, C, R_all, cand, cand_cap, st);
  DetCandArgs a = {};
  a.R_all = R_all; a.slots_per_image = K; a.classes_per_source = C; a.cand_cap = cand_cap; a.num_segs = S; a.pass = pass;
  a.cand = static_cast<char*>(cand);
  a.nms = det_nms_of(nms);
  for (int o = 0; o < num_sources; ++o) a.src[o] = src[o];
  for (int s0 = 0; s0 < S; s0 += kSegsPerLaunch) {
    const int ns = S - s0 < kSegsPerLaunch ? S - s0 : kSegsPerLaunch;
    a.s0 = s0;
    for (int j = 0; j < ns; ++j) {
      a.seg[j] = det_seg_of(desc[s0 + j], src[0].cascade, det_thr);
      a.view[j] = DetView{0.0, 0.0, 0, 0};
      if (view) { const mscnn_detections_view& v = view[(s0 + j) / K]; a.view[j] = DetView{v.off_x, v.off_y, v.flip_x, 1}; }
    }
    if (nms_has_thr(nms)) det_cand_add_thr_kernel<<<ns, kCandThreads, 0, st>>>(a);
    else det_cand_add_kernel<<<ns, kCandThreads, 0, st>>>(a);
    MSCNN_POST_LAUNCH();
  }
  return MSCNN_OK;
}

// what list_of must be in the views forms (checked in front of everything the plain forms check)
static int det_list_of_checked(const char* name, const int* list_of, int num_images, int num_lists) {
  MSCNN_REQUIRE(list_of, "%s: null pointer (list_of)", name);
  MSCNN_REQUIRE(num_lists >= 1, "%s: num_lists %d < 1", name, num_lists);
  for (int b = 0; b < num_images; ++b)
    MSCNN_REQUIRE(list_of[b] >= 0 && list_of[b] < num_lists, "%s: image %d: list_of %d outside [0, %d)", name, b, list_of[b], num_lists);
  return MSCNN_OK;
}

// the plain add and its views form (list_of != NULL)
static int det_cand_add_plain(const char* name, const mscnn_detections_desc* desc, const mscnn_detections_view* view, const int* list_of,
                              int num_lists, const mscnn_nms_params* nms_in, int pass, int num_images, int num_classes,
                              const float* bbox_pred, const float* cls_pred, const float* props, int R_all, void* cand, int cand_cap,
                              void* stream) {
  mscnn_nms_params nms;
  if (int rc = mscnn_nms_params_resolve(nms_in, &nms)) return rc;
  MSCNN_REQUIRE(desc && cand && bbox_pred && cls_pred && props, "%s: null pointer", name);
  MSCNN_REQUIRE(num_images >= 1 && num_classes >= 1, "%s: %d images x %d classes", name, num_images, num_classes);
  MSCNN_REQUIRE((long)num_images * num_classes <= (long)(1 << 24), "%s: %d images x %d classes", name, num_images, num_classes);
  const int S = num_images * num_classes;
  const int ncls = desc[0].ncls;
  for (int s = 0; s < S; ++s)
    MSCNN_REQUIRE(desc[s].ncls == ncls && desc[s].cls_id >= 1 && desc[s].cls_id <= ncls && ncls >= 2, "%s: segment %d: cls_id %d of %d", name, s,
                  desc[s].cls_id, desc[s].ncls);
  const DetSource src = {bbox_pred, cls_pred, props, ncls, 0};
  return det_cand_launch(name, &src, 1, desc, view, 0.f, nms, pass, num_images, num_classes, R_all, cand, cand_cap, stream, list_of, num_lists);
}

extern "C" int mscnn_detections_candidates_add(const mscnn_detections_desc* desc, const mscnn_detections_view* view,
                                               const mscnn_nms_params* nms_in, int pass, int num_images, int num_classes,
                                               const float* bbox_pred, const float* cls_pred, const float* props, int R_all, void* cand,
                                               int cand_cap, void* stream) {
  return det_cand_add_plain("detections_candidates_add", desc, view, nullptr, 0, nms_in, pass, num_images, num_classes, bbox_pred, cls_pred,
                            props, R_all, cand, cand_cap, stream);
}

extern "C" int mscnn_detections_candidates_add_views(const mscnn_detections_desc* desc, const mscnn_detections_view* view, const int* list_of,
                                                     const mscnn_nms_params* nms_in, int pass, int num_images, int num_lists, int num_classes,
                                                     const float* bbox_pred, const float* cls_pred, const float* props, int R_all, void* cand,
                                                     int cand_cap, void* stream) {
  const char* name = "detections_candidates_add_views";
  MSCNN_REQUIRE(num_images >= 1 && num_classes >= 1, "%s: %d images x %d classes", name, num_images, num_classes);
  if (int rc = det_list_of_checked(name, list_of, num_images, num_lists)) return rc;
  return det_cand_add_plain(name, desc, view, list_of, num_lists, nms_in, pass, num_images, num_classes, bbox_pred, cls_pred, props, R_all, cand,
                            cand_cap, stream);
}

// the cascade add and its views form (list_of != NULL)
static int det_cand_add_cascade(const char* name, const mscnn_detections_desc* desc, const mscnn_detections_view* view, const int* list_of,
                                int num_lists, float det_thr, const mscnn_nms_params* nms_in, int pass, int num_images, int num_outputs,
                                int num_classes, const mscnn_cascade_output* outputs, int R_all, void* cand, int cand_cap, void* stream) {
  mscnn_nms_params nms;
  if (int rc = mscnn_nms_params_resolve(nms_in, &nms)) return rc;
  MSCNN_REQUIRE(nms.det_thr == 0.f, "%s: nms params det_thr %g is the plain stage's: the cascade stage takes its det_thr as an argument", name,
                (double)nms.det_thr);
  MSCNN_REQUIRE(num_outputs >= 1 && num_outputs <= kCascadeMaxOutputs, "%s: %d cascade outputs (1 .. %d)", name, num_outputs,
                kCascadeMaxOutputs);
  MSCNN_REQUIRE(desc && outputs && cand, "%s: null pointer", name);
  MSCNN_REQUIRE(num_images >= 1 && num_classes >= 1, "%s: %d images x %d classes", name, num_images, num_classes);
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
  DetSource src[kCascadeMaxOutputs];
  for (int o = 0; o < num_outputs; ++o) src[o] = DetSource{outputs[o].boxes, outputs[o].cls_prob, outputs[o].props, outputs[o].ncls, 1};
  return det_cand_launch(name, src, num_outputs, desc, view, det_thr, nms, pass, num_images, num_classes, R_all, cand, cand_cap, stream, list_of,
                         num_lists);
}

extern "C" int mscnn_detections_candidates_cascade_add(const mscnn_detections_desc* desc, const mscnn_detections_view* view, float det_thr,
                                                       const mscnn_nms_params* nms_in, int pass, int num_images, int num_outputs,
                                                       int num_classes, const mscnn_cascade_output* outputs, int R_all, void* cand,
                                                       int cand_cap, void* stream) {
  return det_cand_add_cascade("detections_candidates_cascade_add", desc, view, nullptr, 0, det_thr, nms_in, pass, num_images, num_outputs,
                              num_classes, outputs, R_all, cand, cand_cap, stream);
}

extern "C" int mscnn_detections_candidates_cascade_add_views(const mscnn_detections_desc* desc, const mscnn_detections_view* view,
                                                             const int* list_of, float det_thr, const mscnn_nms_params* nms_in, int pass,
                                                             int num_images, int num_lists, int num_outputs, int num_classes,
                                                             const mscnn_cascade_output* outputs, int R_all, void* cand, int cand_cap,
                                                             void* stream) {
  const char* name = "detections_candidates_cascade_add_views";
  MSCNN_REQUIRE(num_images >= 1 && num_classes >= 1, "%s: %d images x %d classes", name, num_images, num_classes);
  if (int rc = det_list_of_checked(name, list_of, num_images, num_lists)) return rc;
  return det_cand_add_cascade(name, desc, view, list_of, num_lists, det_thr, nms_in, pass, num_images, num_outputs, num_classes, outputs, R_all,
                              cand, cand_cap, stream);
}

extern "C" size_t mscnn_detections_merge_workspace_bytes(int num_segments, int cand_cap) {
  if (!cand_shape_ok(num_segments, cand_cap)) return 0;
  if (cand_cap > kMaxK) return det_layout(cand_cap).total;      // one list at a time
  return cand_al((size_t)num_segments * MRG_WORDS * sizeof(int)) +
         (size_t)num_segments * (det_merge_seg_box_bytes(cand_cap) + det_merge_seg_mask_bytes(cand_cap));
}

extern "C" int mscnn_detections_merge_fwd(const double* nms_overlap, const mscnn_nms_params* nms_in, int num_segments, void* cand,
                                          int cand_cap, void* pack_dev, void* workspace, size_t workspace_bytes, void* stream) {
  mscnn_nms_params nms;
  if (int rc = mscnn_nms_params_resolve(nms_in, &nms)) return rc;
  MSCNN_REQUIRE(nms_overlap && cand && pack_dev && workspace, "detections_merge: null pointer");
  const int S = num_segments;
  MSCNN_REQUIRE(S >= 1, "detections_merge: %d segments", S);
  MSCNN_REQUIRE(cand_cap >= 1, "detections_merge: cand_cap %d", cand_cap);
  MSCNN_REQUIRE(cand_shape_ok(S, cand_cap), "detections_merge: %d segments x %d slots is past 2^31 - 1", S, cand_cap);
  for (int s = 0; s < S; ++s) MSCNN_REQUIRE(!(nms_overlap[s] != nms_overlap[s]), "detections_merge: segment %d: nms_overlap is NaN", s);
  MSCNN_REQUIRE_ALIGNED(cand, 16, "detections_merge: cand");
  MSCNN_REQUIRE_ALIGNED(workspace, 16, "detections_merge: workspace");
  MSCNN_REQUIRE_ALIGNED(pack_dev, 16, "detections_merge: pack_dev");
  const bool big = cand_cap > kMaxK;
  // (thr and det_thr were applied by the add calls: of the setting, type and ovr_dnm are read here)
  MSCNN_REQUIRE(!big || (nms.type == MSCNN_NMS_TYPE_MAXG && nms.ovr_dnm == MSCNN_NMS_OVR_UNION),
                "detections_merge: lists of %d slots > %d run the tiled path, which has the default type and ovr_dnm only (got type %d, "
                "ovr_dnm %d)", cand_cap, kMaxK, nms.type, nms.ovr_dnm);
  const size_t need = mscnn_detections_merge_workspace_bytes(S, cand_cap);
  if (workspace_bytes < need) {
    set_error("detections_merge: workspace %zu < %zu", workspace_bytes, need);
    return MSCNN_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  const mscnn_multi_pack_layout PL = mscnn_multi_pack_layout_of(S, S * cand_cap);
  char* pk = static_cast<char*>(pack_dev);
  int* hdr = reinterpret_cast<int*>(pk);
  double* dets = reinterpret_cast<double*>(pk + PL.dets);
  int* ids = reinterpret_cast<int*>(pk + PL.ids);
  char* ws = static_cast<char*>(workspace);
  if (!big) {
    DetMergeArgs a = {};
    a.cand_cap = cand_cap; a.wpr = (cand_cap + 63) / 64; a.num_segs = S;
    a.cand = static_cast<char*>(cand); a.ws = ws;
    a.seg_stride_box = det_merge_seg_box_bytes(cand_cap); a.seg_stride_mask = det_merge_seg_mask_bytes(cand_cap);
    a.hdr = hdr; a.dets = dets; a.ids = ids;
    for (int s0 = 0; s0 < S; s0 += kSegsPerLaunch) {
      const int ns = S - s0 < kSegsPerLaunch ? S - s0 : kSegsPerLaunch;
      a.s0 = s0;
      for (int j = 0; j < ns; ++j) a.overlap[j] = nms_overlap[s0 + j];
      det_merge_sort_kernel<<<ns, kSortThreads, 0, st>>>(a);
      MSCNN_POST_LAUNCH();
      if (nms.ovr_dnm == MSCNN_NMS_OVR_MIN) det_merge_mask_min_kernel<<<dim3(a.wpr, a.wpr, ns), 256, 0, st>>>(a);
      else det_merge_mask_kernel<<<dim3(a.wpr, a.wpr, ns), 256, 0, st>>>(a);
      MSCNN_POST_LAUNCH();
      const size_t lds = (size_t)2 * 64 * a.wpr * sizeof(u64);
      if (nms.type == MSCNN_NMS_TYPE_MAXG) det_merge_scan_emit_kernel<<<ns, 256, lds, st>>>(a);
      else det_merge_color_emit_kernel<<<ns, 256, lds, st>>>(a);
      MSCNN_POST_LAUNCH();
    }
    return MSCNN_OK;
  }
  // one list at a time on the tiled kernels; the list's length comes from its device count (big_nms_tiles' total_k)
  const DetLayout L = det_layout(cand_cap);
  const DetCand c = det_cand_of(static_cast<char*>(cand), S, cand_cap);
  int* cnt = reinterpret_cast<int*>(ws + L.cnt);
  DetBox* sbox = reinterpret_cast<DetBox*>(ws + L.sbox);
  double* sprob = reinterpret_cast<double*>(ws + L.sprob);
  int* ssrc = reinterpret_cast<int*>(ws + L.ssrc);
  u64* mask = reinterpret_cast<u64*>(ws + L.mask);
  u64* keys = reinterpret_cast<u64*>(ws + L.keys);
  int* kidx = reinterpret_cast<int*>(ws + L.kidx);
  for (int s = 0; s < S; ++s) {
    const size_t list = (size_t)s * (size_t)cand_cap;
    det_merge_keys_big_kernel<<<cdiv(L.sortP, 256), 256, 0, st>>>(c.cnt + CAND_WORDS * (size_t)s, c.prob + list, cand_cap, keys, L.sortP, cnt);
    MSCNN_POST_LAUNCH();
    MSCNN_HIP_TRY(big_sort_desc(keys, L.sortP, st));
    det_merge_gather_big_kernel<<<cdiv(cand_cap, 256), 256, 0, st>>>(keys, c.box + list, c.prob + list, c.tag + list, sbox, sprob, ssrc, cnt);
    MSCNN_POST_LAUNCH();
    const double overlap = nms_overlap[s];
    auto launch_mask = [&](const DetBox* tile, const int* tile_n) {
      det_mask_kernel<<<dim3(kTileWords, kTileWords), 256, 0, st>>>(tile, tile_n, overlap, mask, kTileWords);
    };
    MSCNN_HIP_TRY((big_nms_tiles<DetTr>(sbox, cnt + DC_N, 0, cand_cap, DetTr::Params{overlap}, mask, reinterpret_cast<u64*>(ws + L.rinit), kidx,
                                        reinterpret_cast<DetBox*>(ws + L.kbox), cnt + DC_BIG, launch_mask, st)));
    det_emit_big_kernel<<<cdiv(cand_cap, 256), 256, 0, st>>>(kidx, cnt + DC_BIG, sbox, sprob, ssrc, dets + 5 * list, ids + list,
                                                             hdr + MSCNN_MULTI_PACK_WORDS * (size_t)(1 + s));
    MSCNN_POST_LAUNCH();
  }
  det_merge_table_big_kernel<<<cdiv(S, 256), 256, 0, st>>>(c.cnt, S, cand_cap, hdr);
  MSCNN_POST_LAUNCH();
  return MSCNN_OK;
}

extern "C" size_t mscnn_detections_merge_soft_workspace_bytes(int num_segments, int cand_cap) {
  if (!cand_shape_ok(num_segments, cand_cap)) return 0;
  // (the launches of a call follow each other on the stream and share the per-segment areas; a list in registers needs none)
  const size_t segs = (size_t)(num_segments < kSegsPerLaunch ? num_segments : kSegsPerLaunch);
  const size_t need = segs * det_soft_seg_bytes(cand_cap);
  return need > cand_al(1) ? need : cand_al(1);
}

extern "C" int mscnn_detections_merge_soft_fwd(const double* nms_overlap, const mscnn_soft_nms_params* soft, int num_segments, void* cand,
                                               int cand_cap, void* pack_dev, void* workspace, size_t workspace_bytes, void* stream) {
  MSCNN_REQUIRE(nms_overlap && soft && cand && pack_dev && workspace, "detections_merge_soft: null pointer");
  const int S = num_segments;
  MSCNN_REQUIRE(S >= 1, "detections_merge_soft: %d segments", S);
  MSCNN_REQUIRE(cand_cap >= 1, "detections_merge_soft: cand_cap %d", cand_cap);
  MSCNN_REQUIRE(cand_shape_ok(S, cand_cap), "detections_merge_soft: %d segments x %d slots is past 2^31 - 1", S, cand_cap);
  MSCNN_REQUIRE(soft->method == MSCNN_SOFT_NMS_LINEAR || soft->method == MSCNN_SOFT_NMS_GAUSSIAN,
                "detections_merge_soft: method %d is neither %d (linear) nor %d (gaussian)", soft->method, MSCNN_SOFT_NMS_LINEAR,
                MSCNN_SOFT_NMS_GAUSSIAN);
  const double inf = __builtin_inf();
  MSCNN_REQUIRE(soft->method != MSCNN_SOFT_NMS_GAUSSIAN || (soft->sigma > 0 && soft->sigma < inf),
                "detections_merge_soft: sigma %g is not a finite value > 0", soft->sigma);      // (NaN included)
  MSCNN_REQUIRE(soft->score_thr >= 0 && soft->score_thr < inf, "detections_merge_soft: score_thr %g is not a finite value >= 0",
                soft->score_thr);
  MSCNN_REQUIRE(soft->max_out >= 0, "detections_merge_soft: max_out %d", soft->max_out);
  if (soft->method == MSCNN_SOFT_NMS_LINEAR)
    for (int s = 0; s < S; ++s)
      MSCNN_REQUIRE(!(nms_overlap[s] != nms_overlap[s]), "detections_merge_soft: segment %d: nms_overlap is NaN", s);
  MSCNN_REQUIRE_ALIGNED(cand, 16, "detections_merge_soft: cand");
  MSCNN_REQUIRE_ALIGNED(workspace, 16, "detections_merge_soft: workspace");
  MSCNN_REQUIRE_ALIGNED(pack_dev, 16, "detections_merge_soft: pack_dev");
  const size_t need = mscnn_detections_merge_soft_workspace_bytes(S, cand_cap);
  if (workspace_bytes < need) {
    set_error("detections_merge_soft: workspace %zu < %zu", workspace_bytes, need);
    return MSCNN_ERR_WORKSPACE;
  }
  const mscnn_multi_pack_layout PL = mscnn_multi_pack_layout_of(S, S * cand_cap);
  char* pk = static_cast<char*>(pack_dev);
  DetSoftArgs a = {};
  a.cand_cap = cand_cap; a.num_segs = S; a.method = soft->method; a.max_out = soft->max_out;
  a.sigma = soft->sigma; a.score_thr = soft->score_thr;
  a.cand = static_cast<char*>(cand); a.ws = static_cast<char*>(workspace); a.seg_stride = det_soft_seg_bytes(cand_cap);
  a.hdr = reinterpret_cast<int*>(pk);
  a.dets = reinterpret_cast<double*>(pk + PL.dets);
  a.ids = reinterpret_cast<int*>(pk + PL.ids);
  for (int s0 = 0; s0 < S; s0 += kSegsPerLaunch) {
    const int ns = S - s0 < kSegsPerLaunch ? S - s0 : kSegsPerLaunch;
    a.s0 = s0;
    for (int j = 0; j < ns; ++j) a.overlap[j] = nms_overlap[s0 + j];
    det_merge_soft_kernel<<<ns, kSoftThreads, 0, as_stream(stream)>>>(a);
    MSCNN_POST_LAUNCH();
  }
  return MSCNN_OK;
}

extern "C" int mscnn_detections_merge_vote_fwd(const mscnn_vote_params* vote, int num_segments, const void* cand, int cand_cap,
                                               void* pack_dev, void* stream) {
  MSCNN_REQUIRE(vote && cand && pack_dev, "detections_merge_vote: null pointer");
  const int S = num_segments;
  MSCNN_REQUIRE(S >= 1, "detections_merge_vote: %d segments", S);
  MSCNN_REQUIRE(cand_cap >= 1, "detections_merge_vote: cand_cap %d", cand_cap);
  MSCNN_REQUIRE(cand_shape_ok(S, cand_cap), "detections_merge_vote: %d segments x %d slots is past 2^31 - 1", S, cand_cap);
  MSCNN_REQUIRE(vote->thr > 0 && vote->thr < 1, "detections_merge_vote: thr %g is outside (0, 1)", vote->thr);      // (NaN included)
  MSCNN_REQUIRE_ALIGNED(cand, 16, "detections_merge_vote: cand");
  MSCNN_REQUIRE_ALIGNED(pack_dev, 16, "detections_merge_vote: pack_dev");
  const mscnn_multi_pack_layout PL = mscnn_multi_pack_layout_of(S, S * cand_cap);
  char* pk = static_cast<char*>(pack_dev);
  DetVoteArgs a;
  a.num_segs = S; a.cand_cap = cand_cap; a.thr = vote->thr;
  a.cand = const_cast<char*>(static_cast<const char*>(cand));
  a.hdr = reinterpret_cast<const int*>(pk);
  a.dets = reinterpret_cast<double*>(pk + PL.dets);
  det_merge_vote_kernel<<<kVoteBlocks, kVoteThreads, 0, as_stream(stream)>>>(a);
  MSCNN_POST_LAUNCH();
  return MSCNN_OK;
}
