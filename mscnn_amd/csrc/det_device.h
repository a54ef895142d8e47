// What the files of the final detection stage share (gfx950): the row transform, the overlap, the bit matrix, the scan / column-OR and
// the emit as device functions, the candidate buffer's and the per-segment workspace's layout, and the host helpers the entry points
// have in common.  detections.hip (single list, segmented, tiled), det_candidates.hip (the adds), det_merge.hip (merge, vote),
// det_soft.hip (Soft-NMS), det_matrix.hip (Matrix NMS), det_wbf.hip (weighted boxes fusion) and det_seq.hip (Seq-NMS) compile from these lines: one definition each, so no
// two of them can disagree about a bit.
//
// Final stage: the MATLAB post-processing of the net outputs, examples/kitti_car/run_mscnn_detection.m:75-120
//   + utils/bbNms.m:112-126 (nmsMax, greedy, union).  MATLAB semantics restated: single-precision
//   arithmetic until `double([...])`, stable descending sort on prob (ties: lower row first), IoU and
//   threshold test in double, pairs with iw <= 0 or ih <= 0 skipped.
// Same kernel structure as BoxOutput's NMS: parallel bit-matrix + one-wavefront greedy scan.
// bbNms's user knobs (mscnn_nms_params): ovrDnm = 'min' is another denominator in the bit matrix (bbNms.m:121), type = 'max' a
// column-OR of that matrix instead of the greedy scan (bbNms.m:117 with greedy = 0), thr the strict prob > thr of bbNms.m:85.
#pragma once
#include <cmath>
#include "common.h"
#include "box_device.h"
#include "det_rows.h"

namespace mscnn_dev {

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
__device__ __forceinline__ int det_key_row(u64 key) { return (int)(0xffffffffu - (unsigned)(key & 0xffffffffull)); }

// ---- the segments of a batched forward ------------------------------------------------------------------------------------------------
// A source is a blob triple whose ROI rows are grouped by image, the image index in column 0 of props (box_output_layer.cpp:107,
// :156; DecodeBBox copies it, decode_bbox_layer.cpp:110).  The plain stage has one (bbox_pred / cls_pred / proposals_score,
// cascade = 0); the cascade stage one per cascade output (decoded boxes / probabilities / proposals, cascade = 1).
constexpr int kSegsPerLaunch = 32;         // sources and segment parameters travel as kernel arguments (2.3 KB of the 4 KB)
constexpr int kCascadeMaxOutputs = 4;
struct DetSource { const float* boxes; const float* cls; const float* props; int ncls, cascade; };   // row strides: props 6 / 5, boxes 4 ncls / 5
struct DetSeg { float mean[4], stdv[4]; float proposal_thr, ratio_h, ratio_w, org_h, org_w; int cls_id; double nms_overlap; };

// rows [row0, row0 + rows) of source t with segment g's parameters, as det_row takes them
__device__ __forceinline__ DetArgs det_args_of(const DetSource& t, const DetSeg& g, int row0, int rows, const DetNms& nms) {
  const int prop_stride = t.cascade ? 5 : 6, box_stride = t.cascade ? 5 : 4 * t.ncls;
  DetArgs d;
  d.bbox_pred = t.boxes + (size_t)row0 * box_stride; d.cls_pred = t.cls + (size_t)row0 * t.ncls; d.props = t.props + (size_t)row0 * prop_stride;
  d.R = rows; d.ncls = t.ncls; d.cls_id = g.cls_id;
  for (int k = 0; k < 4; ++k) { d.mean[k] = g.mean[k]; d.stdv[k] = g.stdv[k]; }
  d.proposal_thr = g.proposal_thr; d.ratio_h = g.ratio_h; d.ratio_w = g.ratio_w; d.org_h = g.org_h; d.org_w = g.org_w;
  d.cascade = t.cascade;
  d.nms_thr = nms.thr; d.det_thr = t.cascade ? 0.f : nms.det_thr;
  return d;
}

// ---- the overlap of two boxes (bbNms.m:117-124, all in double) ------------------------------------------------------------------------
// A is the earlier box, with as_a = A.w * A.h, xe_a = A.x + A.w, ye_a = A.y + A.h computed once by the caller.  A pair with iw <= 0
// or ih <= 0 does not overlap: the result is a NaN, which fails every comparison a caller makes with the ratio (> overlap, >= thr) as
// a NaN ratio of degenerate boxes does.  kDnmMin: ovrDnm = 'min' -- the denominator is the smaller of the two areas instead of the
// union (bbNms.m:121).  The bit matrix, the tiled path's cross test and the vote call this, and soft_decay (det_soft.hip) spells the
// union form out statement for statement: one statement per operation, the same bits everywhere.
template <bool kDnmMin>
__device__ __forceinline__ double det_overlap(const DetBox& A, double as_a, double xe_a, double ye_a, const DetBox& B) {
  const double iw = fmin(xe_a, B.x + B.w) - fmax(A.x, B.x);
  if (iw <= 0) return __builtin_nan("");
  const double ih = fmin(ye_a, B.y + B.h) - fmax(A.y, B.y);
  if (ih <= 0) return __builtin_nan("");
  double o = iw * ih;
  const double u = kDnmMin ? fmin(as_a, B.w * B.h) : as_a + B.w * B.h - o;
  o = o / u;
  return o;
}

// the tiled path's predicate (nms_large.h): == det_mask_block's test, A the earlier box
struct DetTr {
  typedef DetBox Box;
  struct Params { double overlap; };
  static __device__ __forceinline__ bool over(const DetBox& A, const DetBox& B, const Params& p) {
    return det_overlap<false>(A, A.w * A.h, A.x + A.w, A.y + A.h, B) > p.overlap;
  }
};

// One 64 x 64 block (rb, cb) of the upper-triangular bit matrix over n sorted boxes.
// (256 threads per 64 x 64 block, the four waves split the columns -- as nms_mask_kernel of boxoutput.hip)
// (kDnmMin is a template parameter: the union kernels keep the instructions they had.)
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
      if (det_overlap<kDnmMin>(A, as_a, xe_a, ye_a, B) > overlap) bits |= 1u << (q & 15);
    }
  }
  part[wv][t] = bits;
  __syncthreads();
  if (wv == 0 && i < n)
    mask[(size_t)i * wpr + cb] = (u64)part[0][t] | ((u64)part[1][t] << 16) | ((u64)part[2][t] << 32) | ((u64)part[3][t] << 48);
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

// ---- layouts --------------------------------------------------------------------------------------------------------------------------
// every area of a workspace or of the candidate buffer starts on a multiple of 256 bytes
__host__ __device__ __forceinline__ size_t det_al(size_t v) { return (v + 255) / 256 * 256; }

// The per-segment workspace of the segmented stage and of the merge: [cnt: S x kSliceWords ints], then per segment a box slice
// [sbox][sprob][ssrc] (M rows each; kTmp: and [tbox][tprob], the unsorted rows of the transform), then per segment its bit matrix.
constexpr int kSliceWords = 4;
struct DetSlice { int* cnt; DetBox* sbox; double* sprob; int* ssrc; DetBox* tbox; float* tprob; u64* mask; };
__host__ __device__ __forceinline__ size_t det_slice_box_bytes(int M, bool tmp) {
  const size_t m = (size_t)(M < 1 ? 1 : M);
  return det_al(m * sizeof(DetBox)) + det_al(m * sizeof(double)) + det_al(m * sizeof(int)) +
         (tmp ? det_al(m * sizeof(DetBox)) + det_al(m * sizeof(float)) : 0);
}
__host__ __device__ __forceinline__ size_t det_slice_mask_bytes(int M) {
  const size_t m = (size_t)(M < 1 ? 1 : M);
  return det_al(m * (size_t)((m + 63) / 64) * sizeof(u64));
}
__host__ __device__ __forceinline__ size_t det_slices_bytes(int S, int M, bool tmp) {
  return det_al((size_t)S * kSliceWords * sizeof(int)) + (size_t)S * (det_slice_box_bytes(M, tmp) + det_slice_mask_bytes(M));
}
// (the strides are det_slice_box_bytes / det_slice_mask_bytes of M, computed once on the host)
template <bool kTmp>
__device__ __forceinline__ DetSlice det_slice_of(char* ws, int S, int M, size_t stride_box, size_t stride_mask, int s) {
  char* base = ws + det_al((size_t)S * kSliceWords * sizeof(int));
  char* b = base + (size_t)s * stride_box;
  const size_t a32 = det_al((size_t)M * sizeof(DetBox)), a8 = det_al((size_t)M * sizeof(double)), a4 = det_al((size_t)M * sizeof(int));
  DetSlice p;
  p.cnt = reinterpret_cast<int*>(ws) + (size_t)s * kSliceWords;
  p.sbox = reinterpret_cast<DetBox*>(b);
  p.sprob = reinterpret_cast<double*>(b + a32);
  p.ssrc = reinterpret_cast<int*>(b + a32 + a8);
  p.tbox = kTmp ? reinterpret_cast<DetBox*>(b + a32 + a8 + a4) : nullptr;
  p.tprob = kTmp ? reinterpret_cast<float*>(b + 2 * a32 + a8 + a4) : nullptr;
  p.mask = reinterpret_cast<u64*>(base + (size_t)S * stride_box + (size_t)s * stride_mask);
  return p;
}

// The candidates of several forwards of an image (mscnn_detections_candidates_*).  A segment's list: cand_cap slots of box / prob /
// tag and two ints {rows that wanted in, overflow flag}.
enum { CAND_WANTED = 0, CAND_OVER = 1, CAND_WORDS = 2 };
struct DetCand { int* cnt; DetBox* box; float* prob; int* tag; };      // cnt: CAND_WORDS ints per segment; the lists: cand_cap slots per segment
__host__ __device__ __forceinline__ size_t det_cand_bytes(int S, int cap) {
  const size_t n = (size_t)S * (size_t)cap;
  return det_al((size_t)S * CAND_WORDS * sizeof(int)) + det_al(n * sizeof(DetBox)) + 2 * det_al(n * sizeof(int));
}
__host__ __device__ __forceinline__ DetCand det_cand_of(char* cand, int S, int cap) {
  const size_t n = (size_t)S * (size_t)cap;
  DetCand c;
  c.cnt = reinterpret_cast<int*>(cand);
  char* p = cand + det_al((size_t)S * CAND_WORDS * sizeof(int));
  c.box = reinterpret_cast<DetBox*>(p); p += det_al(n * sizeof(DetBox));
  c.prob = reinterpret_cast<float*>(p); p += det_al(n * sizeof(float));
  c.tag = reinterpret_cast<int*>(p);
  return c;
}
inline bool cand_shape_ok(int S, int cand_cap) { return S >= 1 && cand_cap >= 1 && (long)S * (long)cand_cap <= 0x7fffffffL; }

// the multi pack: header + table, dets, ids (mscnn_multi_pack_layout)
struct DetPack { int* hdr; double* dets; int* ids; };
inline DetPack det_pack_of(void* pack_dev, int S, int cap) {
  const mscnn_multi_pack_layout L = mscnn_multi_pack_layout_of(S, cap);
  char* pk = static_cast<char*>(pack_dev);
  return DetPack{reinterpret_cast<int*>(pk), reinterpret_cast<double*>(pk + L.dets), reinterpret_cast<int*>(pk + L.ids)};
}

// ---- host helpers of the entry points -------------------------------------------------------------------------------------------------
inline bool nms_has_thr(const mscnn_nms_params& r) { return r.thr != -HUGE_VAL || r.det_thr != 0.f; }
inline DetNms det_nms_of(const mscnn_nms_params& r) { return DetNms{r.thr, r.det_thr, r.type, r.ovr_dnm}; }

// cascade: proposal_thr = det_thr (run_cascademscnn.m:115-117), mean 0 / std 1 (not read by the cascade row transform)
inline DetSeg det_seg_of(const mscnn_detections_desc& d, int cascade, float det_thr) {
  DetSeg g;
  for (int k = 0; k < 4; ++k) { g.mean[k] = cascade ? 0.f : d.bbox_mean[k]; g.stdv[k] = cascade ? 1.f : d.bbox_std[k]; }
  g.proposal_thr = cascade ? det_thr : d.proposal_thr; g.cls_id = d.cls_id; g.nms_overlap = d.nms_overlap;
  // MATLAB: single op double -> single (the double operand is converted to single first)
  g.ratio_h = (float)d.ratio_h; g.ratio_w = (float)d.ratio_w; g.org_h = (float)d.org_h; g.org_w = (float)d.org_w;
  return g;
}

// What the segmented stage and the candidate adds check alike about their sources, `name` the entry point in the messages
// (detections.hip).  Plain: desc[S], one ncls for all segments and every cls_id inside it -> the one source.  Cascade: outputs[O]
// (O in 1 .. kCascadeMaxOutputs, checked by the caller) without a null pointer and with >= 2 columns, at most 2^24 segments, every
// cls_id inside its output's columns -> src[O].
int det_plain_source(const char* name, const mscnn_detections_desc* desc, int S, const float* bbox_pred, const float* cls_pred,
                     const float* props, DetSource* src);
int det_cascade_sources(const char* name, const mscnn_detections_desc* desc, int num_images, int num_outputs, int num_classes,
                        const mscnn_cascade_output* outputs, DetSource* src);

// The tiled path for one list of more than kMaxK rows (detections.hip; nms_large.h: the greedy scan over union overlaps, tile after
// tile).  Its workspace is mscnn_detections_workspace_bytes(kcap) bytes; det_tiled_of names the areas the CALLER's key kernel
// fills before det_tiled_nms: keys[0 .. P) = det_key(prob, i) of the list's rows and 0 for padding and filtered rows, cnt[DC_N] = the
// number of non-zero keys, cnt[DC_BIG .. + DC_BIG_WORDS) = 0.  det_tiled_nms sorts the keys, gathers box[i] / prob[i] and the id
// (tag[i], or i itself when tag is NULL) in sorted order, runs the tiles and emits dets / ids / *count_out as the one-pass path does.
enum { DC_N = 0, DC_BIG = 4, DC_BIG_WORDS = 2 };
struct DetTiled { u64* keys; int P; int* cnt; DetBox* tbox; float* tprob; };      // tbox / tprob: room for kcap unsorted rows
DetTiled det_tiled_of(void* workspace, int kcap);
int det_tiled_nms(void* workspace, int kcap, const DetBox* box, const float* prob, const int* tag, double overlap, double* dets,
                  int* ids, int* count_out, hipStream_t st);
// the gather of the tiled path alone (detections.hip): sbox / sprob / ssrc[i] = box / prob / tag of det_key_row(keys[i]), i < cnt[DC_N]
void det_tiled_gather(const u64* keys, const DetBox* box, const float* prob, const int* tag, DetBox* sbox, double* sprob, int* ssrc,
                      const int* cnt, int kcap, hipStream_t st);

// ---- the merge's sort, shared with the Matrix NMS, the WBF and Seq-NMS (det_merge.hip launches; det_matrix.hip, det_wbf.hip and det_seq.hip read the slices) ----
// lists of at most kMaxK slots: every segment in one pass, kSegsPerLaunch segments per launch
struct DetMergeArgs {
  int cand_cap, wpr, num_segs, s0;
  char* cand; char* ws; size_t seg_stride_box, seg_stride_mask;      // workspace: per-segment slices (det_slice_of)
  DetPack pack;
  double overlap[kSegsPerLaunch];
};
enum { MRG_N = 0, MRG_WANTED = 1, MRG_OVER = 2 };      // the segment's kSliceWords workspace words
__device__ __forceinline__ DetSlice det_merge_slice(const DetMergeArgs& a, int s) {
  return det_slice_of<false>(a.ws, a.num_segs, a.cand_cap, a.seg_stride_box, a.seg_stride_mask, s);
}
// det_merge_sort_kernel on segments [a.s0, a.s0 + ns): the slice's cnt words, sbox / sprob / ssrc in det_key order, the pack's header
void det_merge_sort_launch(const DetMergeArgs& a, int ns, hipStream_t st);
// det_merge_keys_big_kernel on one list of more than kMaxK slots: keys[0 .. P), cnt[DC_N], cnt[DC_BIG ..] = 0
void det_merge_keys_big_launch(const int* lcnt, const float* prob, int cap, u64* keys, int P, int* cnt, hipStream_t st);

}  // namespace mscnn_dev
