// Matrix NMS over the merged candidates (mscnn_detections_merge_matrix_fwd; Wang et al., "SOLOv2", NeurIPS 2020, Algorithm 1): the
// score decay of Soft-NMS without its serial picks.  A list is sorted by the merge's own sort (det_merge_sort_launch, or key kernel +
// big_sort_desc + det_tiled_gather above kMaxK slots); then
//   comp   c_i = max over k < i of r_ki                              (thread = column i, partial maxima per row split)
//   decay  d_j = min over i < j of (1 - r_ij) / (1 - c_i), or g_j    (thread = column j, c_i combined while a tile is staged)
//   score  score'_j = s_j * d_j  resp.  s_j * exp(-g_j)              (ONE exp per candidate)
//   rank   the number of kept candidates that precede j in the output order (thread = column j, partial counts per row split)
//   emit   the count by ballot / popcount, row j to its position when that is below the count, the table entry
// A workgroup of kMxTile threads owns kMxTile columns and streams tiles of kMxTile sorted rows through LDS (32-byte boxes, 8 KB; in
// the decay pass 2 KB of 1 - c_i resp. c_i * c_i beside them); the row tiles of a column block go round `splits` workgroups, whose
// partial max / min / count meet in the workspace.  Max and min of non-NaN doubles and integer sums are exact, so the split decides
// no bit; the launch boundary is the only ordering used.  r_ij is recomputed in the decay pass: no n x n matrix is stored.  Every
// loop bound that guards a barrier is a kernel argument, a block index or the list's device count, the same in all threads; no
// atomics, nothing spins, no workgroup waits on another.
#include "det_device.h"
#include "nms_large.h"

namespace {
using namespace mscnn_dev;

constexpr int kMxTile = 256;      // columns of a workgroup = rows of a staged tile
constexpr int kMxSplit = 8;       // row splits of a column block at the most
constexpr int kMxMaxCap = 1 << 30;      // big_sort_desc's power of two is an int

struct MxArgs {
  int cand_cap, num_segs, s0, method, max_out, splits, big;
  double sigma, score_thr;
  char* cand;
  char* ws; size_t seg_stride_box;      // lists of at most kMaxK slots: the merge's slices (det_slice_of, no bit matrix behind them)
  const int* bcnt; const DetBox* bsbox; const double* bsprob; const int* bssrc;      // a longer list: the one at hand, sorted
  char* pass; size_t pass_stride, part_stride;      // per segment of a launch: score'[cap], then 2 x splits partial rows (part_stride doubles each)
  DetPack pack;
};
struct MxList { int n; const DetBox* sbox; const double* sprob; const int* ssrc; double* score; double* pa; double* pb; };

__host__ __device__ __forceinline__ int mx_splits(int cap) {
  const int tiles = (int)(((long)cap + kMxTile - 1) / kMxTile);
  return tiles < kMxSplit ? tiles : kMxSplit;
}
__host__ __device__ __forceinline__ size_t mx_pass_bytes(int cap) {
  return (size_t)(1 + 2 * mx_splits(cap)) * det_al((size_t)cap * sizeof(double));
}
inline size_t mx_big_sort_bytes(int cap) {      // [cnt][keys][sbox][sprob][ssrc] of the list at hand
  return 256 + det_al((size_t)big_sort_pow2(cap) * sizeof(u64)) + det_al((size_t)cap * sizeof(DetBox)) + det_al((size_t)cap * sizeof(double)) +
         det_al((size_t)cap * sizeof(int));
}
inline size_t mx_small_sort_bytes(int S, int cap) {
  return det_al((size_t)S * kSliceWords * sizeof(int)) + (size_t)S * det_slice_box_bytes(cap, false);
}

// segment j of the launch: its sorted list and its pass areas
__device__ __forceinline__ MxList mx_list(const MxArgs& a, int j) {
  MxList L;
  if (a.big) {
    L.n = a.bcnt[DC_N]; L.sbox = a.bsbox; L.sprob = a.bsprob; L.ssrc = a.bssrc;
  } else {
    const DetSlice p = det_slice_of<false>(a.ws, a.num_segs, a.cand_cap, a.seg_stride_box, 0, a.s0 + j);
    L.n = p.cnt[MRG_N]; L.sbox = p.sbox; L.sprob = p.sprob; L.ssrc = p.ssrc;
  }
  L.n = L.n < 0 ? 0 : (L.n > a.cand_cap ? a.cand_cap : L.n);
  char* w = a.pass + (size_t)j * a.pass_stride;
  L.score = reinterpret_cast<double*>(w);
  L.pa = L.score + a.part_stride;
  L.pb = L.pa + (size_t)a.splits * a.part_stride;
  return L;
}

// r_ij of the contract, A the higher-ranked box: det_overlap<false>, its NaN (no overlap, or a NaN ratio) mapped to 0.0
__device__ __forceinline__ double mx_ratio(const DetBox& A, const DetBox& B) {
  const double r = det_overlap<false>(A, A.w * A.h, A.x + A.w, A.y + A.h, B);
  return r != r ? 0.0 : r;
}

// grid (column blocks, splits, segments): pa[split][i] = max over this split's rows k < i of r_ki, from 0.0
__global__ __launch_bounds__(kMxTile) void det_matrix_comp_kernel(MxArgs a) {
  __shared__ DetBox tbox[kMxTile];
  const int cb = blockIdx.x, rs = blockIdx.y, tid = threadIdx.x;
  const MxList L = mx_list(a, blockIdx.z);
  if (cb * kMxTile >= L.n) return;
  const int col = cb * kMxTile + tid;
  const bool live = col < L.n;
  const DetBox B = live ? L.sbox[col] : DetBox{0.0, 0.0, 0.0, 0.0};
  double c = 0.0;
  for (int rt = rs; rt <= cb; rt += a.splits) {
    const int i0 = rt * kMxTile, tn = min(kMxTile, L.n - i0);
    __syncthreads();      // (every wave is done with the tile before)
    if (tid < tn) tbox[tid] = L.sbox[i0 + tid];
    __syncthreads();
    if (!live) continue;
    const int qn = min(tn, col - i0);      // rows above the diagonal only
    for (int q = 0; q < qn; ++q) c = fmax(c, mx_ratio(tbox[q], B));
  }
  if (live) L.pa[(size_t)rs * a.part_stride + col] = c;
}

// grid as above: pb[split][j] = min over this split's rows i < j of (1.0 - r_ij) / (1.0 - c_i) from 1.0 (linear), or the max of
// (r_ij * r_ij - c_i * c_i) / sigma from 0.0 (gaussian); c_i = the max of pa's splits, combined as the tile is staged
template <bool kLinear>
__device__ __forceinline__ void mx_decay(const MxArgs& a) {
  __shared__ DetBox tbox[kMxTile];
  __shared__ double tq[kMxTile];      // linear: 1.0 - c_i; gaussian: c_i * c_i
  const int cb = blockIdx.x, rs = blockIdx.y, tid = threadIdx.x;
  const MxList L = mx_list(a, blockIdx.z);
  if (cb * kMxTile >= L.n) return;
  const int col = cb * kMxTile + tid;
  const bool live = col < L.n;
  const DetBox B = live ? L.sbox[col] : DetBox{0.0, 0.0, 0.0, 0.0};
  double v = kLinear ? 1.0 : 0.0;
  for (int rt = rs; rt <= cb; rt += a.splits) {
    const int i0 = rt * kMxTile, tn = min(kMxTile, L.n - i0);
    __syncthreads();
    if (tid < tn) {
      tbox[tid] = L.sbox[i0 + tid];
      double c = 0.0;
      for (int k = 0; k < a.splits; ++k) c = fmax(c, L.pa[(size_t)k * a.part_stride + i0 + tid]);
      tq[tid] = kLinear ? 1.0 - c : c * c;
    }
    __syncthreads();
    if (!live) continue;
    const int qn = min(tn, col - i0);
    for (int q = 0; q < qn; ++q) {
      const double r = mx_ratio(tbox[q], B);
      if (kLinear) {
        const double den = tq[q];
        if (den > 0) v = fmin(v, (1.0 - r) / den);      // (not > 0: an exact duplicate of a higher-ranked box, skipped)
      } else {
        v = fmax(v, (r * r - tq[q]) / a.sigma);
      }
    }
  }
  if (live) L.pb[(size_t)rs * a.part_stride + col] = v;
}
__global__ __launch_bounds__(kMxTile) void det_matrix_decay_linear_kernel(MxArgs a) { mx_decay<true>(a); }
__global__ __launch_bounds__(kMxTile) void det_matrix_decay_gauss_kernel(MxArgs a) { mx_decay<false>(a); }

// grid (column blocks, segments): score'_j = s_j * d_j resp. s_j * exp(-g_j)  (j = 0: d = 1.0, g = 0.0 -- s_0 bit for bit)
__global__ __launch_bounds__(kMxTile) void det_matrix_score_kernel(MxArgs a) {
  const MxList L = mx_list(a, blockIdx.y);
  const int col = blockIdx.x * kMxTile + threadIdx.x;
  if (col >= L.n) return;
  const bool linear = a.method == MSCNN_MATRIX_NMS_LINEAR;
  double v = linear ? 1.0 : 0.0;
  for (int k = 0; k < a.splits; ++k) {
    const double p = L.pb[(size_t)k * a.part_stride + col];
    v = linear ? fmin(v, p) : fmax(v, p);
  }
  const double s = L.sprob[col];
  L.score[col] = linear ? s * v : s * exp(-v);
}

// what the output order compares: score' of a kept candidate, -inf of one under the threshold (a NaN included)
__device__ __forceinline__ double mx_rank_value(double s, double thr) { return s >= thr ? s : -__builtin_inf(); }

// grid (column blocks, splits, segments): the number of this split's candidates that precede j -- the larger score', then the
// lower sorted position -- as an int in pb[split][j]'s place (score' was combined out of pb by the launch before)
__global__ __launch_bounds__(kMxTile) void det_matrix_rank_kernel(MxArgs a) {
  __shared__ double tv[kMxTile];
  const int cb = blockIdx.x, rs = blockIdx.y, tid = threadIdx.x;
  const MxList L = mx_list(a, blockIdx.z);
  if (cb * kMxTile >= L.n) return;
  const int col = cb * kMxTile + tid;
  const bool live = col < L.n;
  const double my = live ? mx_rank_value(L.score[col], a.score_thr) : 0.0;
  const int tiles = (L.n + kMxTile - 1) / kMxTile;
  int before = 0;
  for (int rt = rs; rt < tiles; rt += a.splits) {
    const int i0 = rt * kMxTile, tn = min(kMxTile, L.n - i0);
    __syncthreads();
    if (tid < tn) tv[tid] = mx_rank_value(L.score[i0 + tid], a.score_thr);
    __syncthreads();
    if (!live) continue;
    for (int q = 0; q < tn; ++q) {
      const double o = tv[q];
      before += (o > my || (o == my && i0 + q < col)) ? 1 : 0;
    }
  }
  if (live) reinterpret_cast<int*>(L.pb)[(size_t)rs * a.part_stride + col] = before;
}

// grid (column blocks, segments): count = the kept candidates (ballot / popcount, every workgroup for itself), bounded by max_out;
// row j to pack row s * cand_cap + its position when that is below the count; column block 0 writes the table entry (and the header)
__global__ __launch_bounds__(kMxTile) void det_matrix_emit_kernel(MxArgs a) {
  __shared__ int wsum[kMxTile / 64];
  const int cb = blockIdx.x, j = blockIdx.y, s = a.s0 + j, tid = threadIdx.x;
  const MxList L = mx_list(a, j);
  const size_t list = (size_t)s * (size_t)a.cand_cap;
  if (cb == 0 && tid == 0) {
    const DetCand c = det_cand_of(a.cand, a.num_segs, a.cand_cap);      // (read only)
    const int wanted = c.cnt[CAND_WORDS * (size_t)s + CAND_WANTED], over = c.cnt[CAND_WORDS * (size_t)s + CAND_OVER];
    int* ent = a.pack.hdr + MSCNN_MULTI_PACK_WORDS * (size_t)(1 + s);
    if (s == 0) { a.pack.hdr[0] = a.num_segs; a.pack.hdr[1] = a.cand_cap; a.pack.hdr[2] = a.num_segs * a.cand_cap; a.pack.hdr[3] = 0; }
    ent[1] = wanted; ent[2] = (int)list; ent[3] = 0;
    if (over || wanted > a.cand_cap) ent[0] = -1;      // the list overflowed (its n is 0): nothing else of it is written
    else if (L.n == 0) ent[0] = 0;
  }
  if (cb * kMxTile >= L.n) return;
  int kept = 0;
  for (int i0 = 0; i0 < L.n; i0 += kMxTile) {
    const int i = i0 + tid;
    kept += __popcll(__ballot(i < L.n && L.score[i] >= a.score_thr));      // (the wave's, the same in its 64 lanes)
  }
  if ((tid & 63) == 0) wsum[tid >> 6] = kept;
  __syncthreads();
  int count = 0;
  for (int w = 0; w < kMxTile / 64; ++w) count += wsum[w];
  if (a.max_out > 0 && count > a.max_out) count = a.max_out;
  if (cb == 0 && tid == 0) a.pack.hdr[MSCNN_MULTI_PACK_WORDS * (size_t)(1 + s)] = count;
  const int col = cb * kMxTile + tid;
  if (col >= L.n) return;
  const double sc = L.score[col];
  if (!(sc >= a.score_thr)) return;
  int pos = 0;
  for (int k = 0; k < a.splits; ++k) pos += reinterpret_cast<const int*>(L.pb)[(size_t)k * a.part_stride + col];
  if (pos >= count) return;
  const DetBox b = L.sbox[col];
  double* d = a.pack.dets + 5 * (list + (size_t)pos);
  d[0] = b.x; d[1] = b.y; d[2] = b.w; d[3] = b.h; d[4] = sc;
  a.pack.ids[list + (size_t)pos] = L.ssrc[col];
}

inline bool mx_shape_ok(int S, int cap) { return cand_shape_ok(S, cap) && cap <= kMxMaxCap; }
}  // namespace

using namespace mscnn;

extern "C" size_t mscnn_detections_merge_matrix_workspace_bytes(int num_segments, int cand_cap) {
  if (!mx_shape_ok(num_segments, cand_cap)) return 0;
  // (the launches of a call follow each other on the stream and share the pass areas; a list above kMaxK slots is sorted alone)
  const size_t segs = cand_cap > kMaxK ? 1 : (size_t)(num_segments < kSegsPerLaunch ? num_segments : kSegsPerLaunch);
  const size_t sort = cand_cap > kMaxK ? mx_big_sort_bytes(cand_cap) : mx_small_sort_bytes(num_segments, cand_cap);
  return sort + segs * mx_pass_bytes(cand_cap);
}

extern "C" int mscnn_detections_merge_matrix_fwd(const mscnn_matrix_nms_params* mx, int num_segments, void* cand, int cand_cap,
                                                 void* pack_dev, void* workspace, size_t workspace_bytes, void* stream) {
  MSCNN_REQUIRE(mx && cand && pack_dev && workspace, "detections_merge_matrix: null pointer");
  const int S = num_segments;
  MSCNN_REQUIRE(S >= 1, "detections_merge_matrix: %d segments", S);
  MSCNN_REQUIRE(cand_cap >= 1, "detections_merge_matrix: cand_cap %d", cand_cap);
  MSCNN_REQUIRE(cand_shape_ok(S, cand_cap), "detections_merge_matrix: %d segments x %d slots is past 2^31 - 1", S, cand_cap);
  MSCNN_REQUIRE(cand_cap <= kMxMaxCap, "detections_merge_matrix: cand_cap %d is past the sort's 2^30 keys", cand_cap);
  MSCNN_REQUIRE(mx->method == MSCNN_MATRIX_NMS_LINEAR || mx->method == MSCNN_MATRIX_NMS_GAUSSIAN,
                "detections_merge_matrix: method %d is neither %d (linear) nor %d (gaussian)", mx->method, MSCNN_MATRIX_NMS_LINEAR,
                MSCNN_MATRIX_NMS_GAUSSIAN);
  const double inf = __builtin_inf();
  MSCNN_REQUIRE(mx->method != MSCNN_MATRIX_NMS_GAUSSIAN || (mx->sigma > 0 && mx->sigma < inf),
                "detections_merge_matrix: sigma %g is not a finite value > 0", mx->sigma);      // (NaN included)
  MSCNN_REQUIRE(mx->score_thr >= 0 && mx->score_thr < inf, "detections_merge_matrix: score_thr %g is not a finite value >= 0", mx->score_thr);
  MSCNN_REQUIRE(mx->max_out >= 0, "detections_merge_matrix: max_out %d", mx->max_out);
  MSCNN_REQUIRE_ALIGNED(cand, 16, "detections_merge_matrix: cand");
  MSCNN_REQUIRE_ALIGNED(workspace, 16, "detections_merge_matrix: workspace");
  MSCNN_REQUIRE_ALIGNED(pack_dev, 16, "detections_merge_matrix: pack_dev");
  const size_t need = mscnn_detections_merge_matrix_workspace_bytes(S, cand_cap);
  if (workspace_bytes < need) {
    set_error("detections_merge_matrix: workspace %zu < %zu", workspace_bytes, need);
    return MSCNN_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  const bool big = cand_cap > kMaxK;
  const bool linear = mx->method == MSCNN_MATRIX_NMS_LINEAR;
  char* ws = static_cast<char*>(workspace);
  MxArgs a = {};
  a.cand_cap = cand_cap; a.num_segs = S; a.method = mx->method; a.max_out = mx->max_out; a.splits = mx_splits(cand_cap); a.big = big ? 1 : 0;
  a.sigma = mx->sigma; a.score_thr = mx->score_thr;
  a.cand = static_cast<char*>(cand);
  a.pass = ws + (big ? mx_big_sort_bytes(cand_cap) : mx_small_sort_bytes(S, cand_cap));
  a.pass_stride = mx_pass_bytes(cand_cap); a.part_stride = det_al((size_t)cand_cap * sizeof(double)) / sizeof(double);
  a.pack = det_pack_of(pack_dev, S, S * cand_cap);
  const int cbs = cdiv(cand_cap, kMxTile);
  auto passes = [&](int ns) -> int {
    const dim3 split(cbs, a.splits, ns), whole(cbs, ns);
    det_matrix_comp_kernel<<<split, kMxTile, 0, st>>>(a);
    MSCNN_POST_LAUNCH();
    if (linear) det_matrix_decay_linear_kernel<<<split, kMxTile, 0, st>>>(a);
    else det_matrix_decay_gauss_kernel<<<split, kMxTile, 0, st>>>(a);
    MSCNN_POST_LAUNCH();
    det_matrix_score_kernel<<<whole, kMxTile, 0, st>>>(a);
    MSCNN_POST_LAUNCH();
    det_matrix_rank_kernel<<<split, kMxTile, 0, st>>>(a);
    MSCNN_POST_LAUNCH();
    det_matrix_emit_kernel<<<whole, kMxTile, 0, st>>>(a);
    MSCNN_POST_LAUNCH();
    return MSCNN_OK;
  };
  if (!big) {
    DetMergeArgs m = {};      // the merge's sort on its own slices; no bit matrix follows them (stride 0, never touched)
    m.cand_cap = cand_cap; m.wpr = 0; m.num_segs = S; m.cand = a.cand; m.ws = ws;
    m.seg_stride_box = det_slice_box_bytes(cand_cap, false); m.seg_stride_mask = 0; m.pack = a.pack;
    a.ws = ws; a.seg_stride_box = m.seg_stride_box;
    for (int s0 = 0; s0 < S; s0 += kSegsPerLaunch) {
      const int ns = S - s0 < kSegsPerLaunch ? S - s0 : kSegsPerLaunch;
      m.s0 = s0; a.s0 = s0;
      det_merge_sort_launch(m, ns, st);
      MSCNN_POST_LAUNCH();
      if (int rc = passes(ns)) return rc;
    }
    return MSCNN_OK;
  }
  // list after list: the tiled path's key kernel, sort and gather; the list's length is its device count
  const DetCand c = det_cand_of(a.cand, S, cand_cap);
  const int P = big_sort_pow2(cand_cap);
  int* bcnt = reinterpret_cast<int*>(ws);
  char* p = ws + 256;
  u64* keys = reinterpret_cast<u64*>(p); p += det_al((size_t)P * sizeof(u64));
  DetBox* sbox = reinterpret_cast<DetBox*>(p); p += det_al((size_t)cand_cap * sizeof(DetBox));
  double* sprob = reinterpret_cast<double*>(p); p += det_al((size_t)cand_cap * sizeof(double));
  int* ssrc = reinterpret_cast<int*>(p);
  a.bcnt = bcnt; a.bsbox = sbox; a.bsprob = sprob; a.bssrc = ssrc;
  for (int s = 0; s < S; ++s) {
    const size_t list = (size_t)s * (size_t)cand_cap;
    det_merge_keys_big_launch(c.cnt + CAND_WORDS * (size_t)s, c.prob + list, cand_cap, keys, P, bcnt, st);
    MSCNN_POST_LAUNCH();
    MSCNN_HIP_TRY(big_sort_desc(keys, P, st));
    det_tiled_gather(keys, c.box + list, c.prob + list, c.tag + list, sbox, sprob, ssrc, bcnt, cand_cap, st);
    MSCNN_POST_LAUNCH();
    a.s0 = s;
    if (int rc = passes(1)) return rc;
  }
  return MSCNN_OK;
}
