// Weighted boxes fusion over the merged candidates (mscnn_detections_merge_wbf_fwd; Solovyev, Wang, Gabruseva, 2019 / Image and Vision
// Computing 2021): serial in the walked candidates, parallel in the clusters.  A list is sorted by the merge's own sort
// (det_merge_sort_launch, or key kernel + big_sort_desc + det_tiled_gather above kMaxK slots, as det_matrix.hip); then ONE workgroup of
// kWbfThreads owns the list and walks it.  Thread t owns clusters t, t + kWbfThreads, ... for the whole call.  A step: the walked
// candidate's box and score are the same address in every lane (uniform registers); every thread's overlap of that box with the fused
// boxes of its clusters, a butterfly over the 64 lanes of the waves that own a cluster, the wave's best (r, c) into one of two LDS
// buffers, ONE barrier, every thread reads the entries of those waves and finds the same winner; the winner's owner -- or the owner
// of the new cluster C -- updates the five running sums, which only it ever touches and which live in the workspace, and the fused
// box.  The buffers alternate: a thread writes buffer k & 1 for step k + 2 only behind barrier k + 1, which every thread reaches
// behind its reads of step k.  The winner is a maximum under a total order (wbf_better: the larger r, then the lower cluster), so
// nothing depends on the shape of the reduction.  A list of at most kWbfRegs candidates keeps the fused boxes of its clusters in
// registers (kWbfPer per thread); a longer one reads them back from the workspace -- the same det_overlap per cluster, the same
// statements in wbf_join, the same bits.  Behind the walk: conf per cluster, a rank pass over the C clusters through LDS tiles (as
// the Matrix NMS's), the emit.  Every loop bound and every value that guards a barrier is a kernel argument, the list's device count,
// the walked candidate's score (one address for all lanes) or the winner read out of LDS, the same in all threads; a step walks one
// candidate, so the loop runs at most n times; no atomics, nothing spins, no workgroup waits on another.
#include "det_device.h"
#include "nms_large.h"

namespace {
using namespace mscnn_dev;

constexpr int kWbfThreads = 1024, kWbfWaves = kWbfThreads / 64, kWbfPer = 4, kWbfRegs = kWbfThreads * kWbfPer;
constexpr int kWbfNone = 0x7fffffff;      // the cluster of "no match": loses every tie
constexpr int kWbfMaxCap = 1 << 30;       // big_sort_desc's power of two is an int

struct WbfSum { double sw, sx, sy, sW, sH; };      // the running sums of a cluster, in walk order
struct WbfBest { double r; int c; int pad; };

struct WbfArgs {
  int cand_cap, num_segs, s0, conf_type, max_out, big;
  double thr, skip_thr;
  char* cand;
  char* ws; size_t seg_stride_box;      // lists of at most kMaxK slots: the merge's slices (det_slice_of, no bit matrix behind them)
  const int* bcnt; const DetBox* bsbox; const double* bsprob; const int* bssrc;      // a longer list: the one at hand, sorted
  char* walk; size_t walk_stride;      // per segment of a launch: sums, fused boxes, conf, members, first (cand_cap entries each)
  DetPack pack; int* members;
  int expected[kSegsPerLaunch];
};
struct WbfList { int n; const DetBox* sbox; const double* sprob; const int* ssrc; WbfSum* sum; DetBox* fbox; double* conf; int* members; int* first; };

__host__ __device__ __forceinline__ size_t wbf_walk_bytes(int cap) {
  const size_t m = (size_t)cap;
  return det_al(m * sizeof(WbfSum)) + det_al(m * sizeof(DetBox)) + det_al(m * sizeof(double)) + 2 * det_al(m * sizeof(int));
}
inline size_t wbf_big_sort_bytes(int cap) {      // [cnt][keys][sbox][sprob][ssrc] of the list at hand (det_matrix.hip's layout)
  return 256 + det_al((size_t)big_sort_pow2(cap) * sizeof(u64)) + det_al((size_t)cap * sizeof(DetBox)) + det_al((size_t)cap * sizeof(double)) +
         det_al((size_t)cap * sizeof(int));
}
inline size_t wbf_small_sort_bytes(int S, int cap) {
  return det_al((size_t)S * kSliceWords * sizeof(int)) + (size_t)S * det_slice_box_bytes(cap, false);
}

// segment j of the launch: its sorted list and its walk areas
__device__ __forceinline__ WbfList wbf_list(const WbfArgs& a, int j) {
  WbfList L;
  if (a.big) {
    L.n = a.bcnt[DC_N]; L.sbox = a.bsbox; L.sprob = a.bsprob; L.ssrc = a.bssrc;
  } else {
    const DetSlice p = det_slice_of<false>(a.ws, a.num_segs, a.cand_cap, a.seg_stride_box, 0, a.s0 + j);
    L.n = p.cnt[MRG_N]; L.sbox = p.sbox; L.sprob = p.sprob; L.ssrc = p.ssrc;
  }
  L.n = L.n < 0 ? 0 : (L.n > a.cand_cap ? a.cand_cap : L.n);
  const size_t m = (size_t)a.cand_cap;
  char* w = a.walk + (size_t)j * a.walk_stride;
  L.sum = reinterpret_cast<WbfSum*>(w); w += det_al(m * sizeof(WbfSum));
  L.fbox = reinterpret_cast<DetBox*>(w); w += det_al(m * sizeof(DetBox));
  L.conf = reinterpret_cast<double*>(w); w += det_al(m * sizeof(double));
  L.members = reinterpret_cast<int*>(w); w += det_al(m * sizeof(int));
  L.first = reinterpret_cast<int*>(w);
  return L;
}

// the total order of the argmax: the larger r, then the lower cluster
__device__ __forceinline__ bool wbf_better(double ra, int ca, double rb, int cb) { return ra > rb || (ra == rb && ca < cb); }
// step 3 of the contract for one cluster: det_overlap<false> with A = the fused box; a NaN (no overlap, or a NaN ratio) fails r > thr
__device__ __forceinline__ void wbf_match(WbfBest& b, const DetBox& F, const DetBox& B, double thr, int c) {
  const double r = det_overlap<false>(F, F.w * F.h, F.x + F.w, F.y + F.h, B);
  if (r > thr && wbf_better(r, c, b.r, b.c)) { b.r = r; b.c = c; }
}
// the wave's best into every lane: an xor butterfly (a maximum under a total order is idempotent: the shape is free)
__device__ __forceinline__ WbfBest wbf_wave_best(WbfBest b) {
  for (int m = 1; m <= 32; m <<= 1) {
    const double ro = __shfl_xor(b.r, m);
    const int co = __shfl_xor(b.c, m);
    if (wbf_better(ro, co, b.r, b.c)) { b.r = ro; b.c = co; }
  }
  return b;
}
// step 4: a new cluster of candidate (B, s); its fused box is B bit for bit
__device__ __forceinline__ void wbf_open(const WbfList& L, int c, int i, const DetBox& B, double s) {
  L.sum[c] = WbfSum{s, s * B.x, s * B.y, s * B.w, s * B.h};
  L.members[c] = 1; L.first[c] = i;
  L.fbox[c] = B;
}
// step 5: candidate (B, s) joins cluster c -- the product rounded, then the sum; then the four divisions
__device__ __forceinline__ DetBox wbf_join(const WbfList& L, int c, const DetBox& B, double s) {
  WbfSum u = L.sum[c];
  u.sw = u.sw + s;
  u.sx = u.sx + s * B.x; u.sy = u.sy + s * B.y; u.sW = u.sW + s * B.w; u.sH = u.sH + s * B.h;
  L.sum[c] = u;
  L.members[c] = L.members[c] + 1;
  const DetBox F = DetBox{u.sx / u.sw, u.sy / u.sw, u.sW / u.sw, u.sH / u.sw};
  L.fbox[c] = F;
  return F;
}

// steps 2 to 5: the walk.  Returns the number of clusters, the same in every thread.
template <bool kRegs>
__device__ __forceinline__ int wbf_walk(const WbfArgs& a, const WbfList& L, WbfBest (*pick)[kWbfWaves]) {
  const int tid = threadIdx.x, wave = tid >> 6;
  DetBox rf[kWbfPer];      // kRegs: the fused box of cluster tid + q * kWbfThreads
#pragma unroll
  for (int q = 0; q < kWbfPer; ++q) rf[q] = DetBox{0.0, 0.0, 0.0, 0.0};
  int C = 0;
  for (int i = 0; i < L.n; ++i) {
    const double s = L.sprob[i];      // (one address for all lanes)
    if (!(s >= a.skip_thr && s > 0)) break;      // the order makes this the same as filtering (a NaN sorts last and fails)
    const DetBox B = L.sbox[i];
    WbfBest best = {-__builtin_inf(), kWbfNone, 0};
    if (kRegs) {
#pragma unroll
      for (int q = 0; q < kWbfPer; ++q) {
        const int c = tid + q * kWbfThreads;
        if (c < C) wbf_match(best, rf[q], B, a.thr, c);
      }
    } else {
      for (int c = tid; c < C; c += kWbfThreads) wbf_match(best, L.fbox[c], B, a.thr, c);      // (written by this thread)
    }
    const int nw = ((C < kWbfThreads ? C : kWbfThreads) + 63) >> 6;      // the waves that own a cluster
    WbfBest* buf = pick[i & 1];
    if (wave < nw) {
      best = wbf_wave_best(best);
      if ((tid & 63) == 0) buf[wave] = best;
    }
    __syncthreads();
    WbfBest W = {-__builtin_inf(), kWbfNone, 0};
    for (int e = 0; e < nw; ++e) {
      const WbfBest o = buf[e];
      if (wbf_better(o.r, o.c, W.r, W.c)) W = o;
    }
    const int c = W.c == kWbfNone ? C : W.c;      // no cluster above thr: a new one
    if ((c & (kWbfThreads - 1)) == tid) {      // its owner
      DetBox F = B;
      if (W.c == kWbfNone) wbf_open(L, c, i, B, s);
      else F = wbf_join(L, c, B, s);
      if (kRegs) {
        const int q = c / kWbfThreads;
#pragma unroll
        for (int k = 0; k < kWbfPer; ++k) if (q == k) rf[k] = F;
      }
    }
    if (W.c == kWbfNone) ++C;
  }
  return C;
}

// one workgroup per list: table entry, walk, conf, rank, emit
__global__ __launch_bounds__(kWbfThreads) void det_merge_wbf_kernel(WbfArgs a) {
  __shared__ WbfBest pick[2][kWbfWaves];
  __shared__ double tile[kWbfThreads];
  const int j = blockIdx.x, s = a.s0 + j, tid = threadIdx.x;
  const DetCand cd = det_cand_of(a.cand, a.num_segs, a.cand_cap);      // (read only)
  const int wanted = cd.cnt[CAND_WORDS * (size_t)s + CAND_WANTED], over = cd.cnt[CAND_WORDS * (size_t)s + CAND_OVER];
  const size_t list = (size_t)s * (size_t)a.cand_cap;
  int* ent = a.pack.hdr + MSCNN_MULTI_PACK_WORDS * (size_t)(1 + s);
  if (s == 0 && tid == 0) { a.pack.hdr[0] = a.num_segs; a.pack.hdr[1] = a.cand_cap; a.pack.hdr[2] = a.num_segs * a.cand_cap; a.pack.hdr[3] = 0; }
  if (tid == 0) { ent[1] = wanted; ent[2] = (int)list; ent[3] = 0; }
  if (over || wanted > a.cand_cap) { if (tid == 0) ent[0] = -1; return; }      // the list overflowed: nothing else of it is written
  const WbfList L = wbf_list(a, j);
  const int C = L.n <= kWbfRegs ? wbf_walk<true>(a, L, pick) : wbf_walk<false>(a, L, pick);
  const int count = (a.max_out > 0 && C > a.max_out) ? a.max_out : C;
  if (tid == 0) ent[0] = count;
  // step 6, by the cluster's owner (who wrote its sums)
  const int T = a.expected[j];
  for (int c = tid; c < C; c += kWbfThreads) {
    const int m = L.members[c];
    double conf = a.conf_type == MSCNN_WBF_CONF_AVG ? L.sum[c].sw / (double)m : L.sprob[L.first[c]];
    conf = conf * (double)(m < T ? m : T) / (double)T;
    L.conf[c] = conf;
  }
  // step 7: the position of cluster c = the number of clusters before it (the larger conf, then the lower index)
  for (int c0 = 0; c0 < C; c0 += kWbfThreads) {
    const int c = c0 + tid;
    const bool live = c < C;
    int before = 0;
    const double my = live ? L.conf[c] : 0.0;      // (written by this thread)
    for (int t0 = 0; t0 < C; t0 += kWbfThreads) {
      const int tn = min(kWbfThreads, C - t0);
      __syncthreads();      // (the conf of every owner is written; every wave is done with the tile before)
      if (tid < tn) tile[tid] = L.conf[t0 + tid];
      __syncthreads();
      if (!live) continue;
      for (int q = 0; q < tn; ++q) {
        const double o = tile[q];
        before += (o > my || (o == my && t0 + q < c)) ? 1 : 0;
      }
    }
    if (!live || before >= count) continue;
    const DetBox F = L.fbox[c];
    double* d = a.pack.dets + 5 * (list + (size_t)before);
    d[0] = F.x; d[1] = F.y; d[2] = F.w; d[3] = F.h; d[4] = my;
    a.pack.ids[list + (size_t)before] = L.ssrc[L.first[c]];
    if (a.members) a.members[list + (size_t)before] = L.members[c];
  }
}

inline bool wbf_shape_ok(int S, int cap) { return cand_shape_ok(S, cap) && cap <= kWbfMaxCap; }
}  // namespace

using namespace mscnn;

extern "C" size_t mscnn_detections_merge_wbf_workspace_bytes(int num_segments, int cand_cap) {
  if (!wbf_shape_ok(num_segments, cand_cap)) return 0;
  // (the launches of a call follow each other on the stream and share the walk areas; a list above kMaxK slots is sorted alone)
  const size_t segs = cand_cap > kMaxK ? 1 : (size_t)(num_segments < kSegsPerLaunch ? num_segments : kSegsPerLaunch);
  const size_t sort = cand_cap > kMaxK ? wbf_big_sort_bytes(cand_cap) : wbf_small_sort_bytes(num_segments, cand_cap);
  return sort + segs * wbf_walk_bytes(cand_cap);
}

extern "C" int mscnn_detections_merge_wbf_fwd(const mscnn_wbf_params* wbf, const int* expected, int num_segments, void* cand, int cand_cap,
                                              void* pack_dev, int* members_dev, void* workspace, size_t workspace_bytes, void* stream) {
  MSCNN_REQUIRE(wbf && expected && cand && pack_dev && workspace, "detections_merge_wbf: null pointer");
  const int S = num_segments;
  MSCNN_REQUIRE(S >= 1, "detections_merge_wbf: %d segments", S);
  MSCNN_REQUIRE(cand_cap >= 1, "detections_merge_wbf: cand_cap %d", cand_cap);
  MSCNN_REQUIRE(cand_shape_ok(S, cand_cap), "detections_merge_wbf: %d segments x %d slots is past 2^31 - 1", S, cand_cap);
  MSCNN_REQUIRE(cand_cap <= kWbfMaxCap, "detections_merge_wbf: cand_cap %d is past the sort's 2^30 keys", cand_cap);
  MSCNN_REQUIRE(wbf->thr > 0 && wbf->thr < 1, "detections_merge_wbf: thr %g is not inside (0, 1)", wbf->thr);      // (NaN included)
  MSCNN_REQUIRE(wbf->skip_thr >= 0 && wbf->skip_thr < __builtin_inf(), "detections_merge_wbf: skip_thr %g is not a finite value >= 0",
                wbf->skip_thr);
  MSCNN_REQUIRE(wbf->conf_type == MSCNN_WBF_CONF_AVG || wbf->conf_type == MSCNN_WBF_CONF_MAX,
                "detections_merge_wbf: conf_type %d is neither %d (avg) nor %d (max)", wbf->conf_type, MSCNN_WBF_CONF_AVG, MSCNN_WBF_CONF_MAX);
  MSCNN_REQUIRE(wbf->max_out >= 0, "detections_merge_wbf: max_out %d", wbf->max_out);
  for (int s = 0; s < S; ++s) MSCNN_REQUIRE(expected[s] >= 1, "detections_merge_wbf: segment %d: expected %d", s, expected[s]);
  MSCNN_REQUIRE_ALIGNED(cand, 16, "detections_merge_wbf: cand");
  MSCNN_REQUIRE_ALIGNED(workspace, 16, "detections_merge_wbf: workspace");
  MSCNN_REQUIRE_ALIGNED(pack_dev, 16, "detections_merge_wbf: pack_dev");
  MSCNN_REQUIRE_ALIGNED(members_dev, 4, "detections_merge_wbf: members_dev");
  const size_t need = mscnn_detections_merge_wbf_workspace_bytes(S, cand_cap);
  if (workspace_bytes < need) {
    set_error("detections_merge_wbf: workspace %zu < %zu", workspace_bytes, need);
    return MSCNN_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  const bool big = cand_cap > kMaxK;
  char* ws = static_cast<char*>(workspace);
  WbfArgs a = {};
  a.cand_cap = cand_cap; a.num_segs = S; a.conf_type = wbf->conf_type; a.max_out = wbf->max_out; a.big = big ? 1 : 0;
  a.thr = wbf->thr; a.skip_thr = wbf->skip_thr;
  a.cand = static_cast<char*>(cand);
  a.walk = ws + (big ? wbf_big_sort_bytes(cand_cap) : wbf_small_sort_bytes(S, cand_cap));
  a.walk_stride = wbf_walk_bytes(cand_cap);
  a.pack = det_pack_of(pack_dev, S, S * cand_cap);
  a.members = members_dev;
  if (!big) {
    DetMergeArgs m = {};      // the merge's sort on its own slices; no bit matrix follows them (stride 0, never touched)
    m.cand_cap = cand_cap; m.wpr = 0; m.num_segs = S; m.cand = a.cand; m.ws = ws;
    m.seg_stride_box = det_slice_box_bytes(cand_cap, false); m.seg_stride_mask = 0; m.pack = a.pack;
    a.ws = ws; a.seg_stride_box = m.seg_stride_box;
    for (int s0 = 0; s0 < S; s0 += kSegsPerLaunch) {
      const int ns = S - s0 < kSegsPerLaunch ? S - s0 : kSegsPerLaunch;
      m.s0 = s0; a.s0 = s0;
      for (int j = 0; j < ns; ++j) a.expected[j] = expected[s0 + j];
      det_merge_sort_launch(m, ns, st);
      MSCNN_POST_LAUNCH();
      det_merge_wbf_kernel<<<ns, kWbfThreads, 0, st>>>(a);
      MSCNN_POST_LAUNCH();
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
    a.s0 = s; a.expected[0] = expected[s];
    det_merge_wbf_kernel<<<1, kWbfThreads, 0, st>>>(a);
    MSCNN_POST_LAUNCH();
  }
  return MSCNN_OK;
}
