// One NMS over the candidate lists of det_candidates.hip (mscnn_detections_merge_fwd) and box voting behind it
// (mscnn_detections_merge_vote_fwd).  `merge` sorts each list by det_key(prob, candidate index) and runs the final stage's bit
// matrix and scan / column-OR (det_device.h) over it; a list of more than kMaxK slots goes through the tiled path of detections.hip.
// One workgroup owns a segment's list in every kernel: no atomics on global memory, no workgroup waits on another.
#include "det_device.h"

namespace {
using namespace mscnn_dev;

// -- merge, lists of at most kMaxK slots: every segment in one pass, three launches per kSegsPerLaunch segments (DetMergeArgs:
// det_device.h)

// one workgroup per segment: keys of the list's candidates, sort, the sorted boxes.  A list that overflowed is not run (n = 0).
__global__ __launch_bounds__(kSortThreads) void det_merge_sort_kernel(DetMergeArgs a) {
  __shared__ u64 sk[kSortCap];
  const int j = blockIdx.x, s = a.s0 + j, tid = threadIdx.x;
  const DetCand c = det_cand_of(a.cand, a.num_segs, a.cand_cap);
  const DetSlice p = det_merge_slice(a, s);
  const int wanted = c.cnt[CAND_WORDS * (size_t)s + CAND_WANTED], over = c.cnt[CAND_WORDS * (size_t)s + CAND_OVER];
  const int n = (over || wanted > a.cand_cap) ? 0 : (wanted < 0 ? 0 : wanted);
  if (s == 0 && tid == 0) { a.pack.hdr[0] = a.num_segs; a.pack.hdr[1] = a.cand_cap; a.pack.hdr[2] = a.num_segs * a.cand_cap; a.pack.hdr[3] = 0; }
  if (tid == 0) { p.cnt[MRG_N] = n; p.cnt[MRG_WANTED] = wanted; p.cnt[MRG_OVER] = (over || wanted > a.cand_cap) ? 1 : 0; }
  if (n == 0) return;
  const size_t list = (size_t)s * (size_t)a.cand_cap;
  int P = 1;
  while (P < n) P <<= 1;
  for (int i = tid; i < P; i += kSortThreads) sk[i] = i < n ? det_key(c.prob[list + i], i) : 0ull;
  __syncthreads();
  bitonic_desc(sk, P, tid, kSortThreads);
  for (int i = tid; i < n; i += kSortThreads) {
    const int k = det_key_row(sk[i]);
    p.sbox[i] = c.box[list + k];
    p.sprob[i] = (double)c.prob[list + k];
    p.ssrc[i] = c.tag[list + k];
  }
}

template <bool kDnmMin>
__device__ __forceinline__ void det_merge_mask(const DetMergeArgs& a) {
  const int j = blockIdx.z, s = a.s0 + j;
  const DetSlice p = det_merge_slice(a, s);
  det_mask_block<kDnmMin>(p.sbox, p.cnt[MRG_N], a.overlap[j], p.mask, a.wpr, blockIdx.y, blockIdx.x);
}
__global__ __launch_bounds__(256) void det_merge_mask_kernel(DetMergeArgs a) { det_merge_mask<false>(a); }
__global__ __launch_bounds__(256) void det_merge_mask_min_kernel(DetMergeArgs a) { det_merge_mask<true>(a); }

// table entry {count (-1: the list overflowed), rows that wanted in, first pack row, 0}
template <bool kGreedy>
__device__ __forceinline__ void det_merge_emit(const DetMergeArgs& a, u64* dyn_lds) {
  const int j = blockIdx.x, s = a.s0 + j;
  const DetSlice p = det_merge_slice(a, s);
  int* ent = a.pack.hdr + MSCNN_MULTI_PACK_WORDS * (size_t)(1 + s);
  const size_t slot = (size_t)s * (size_t)a.cand_cap;
  if (threadIdx.x == 0) { ent[1] = p.cnt[MRG_WANTED]; ent[2] = (int)slot; ent[3] = 0; }
  if (p.cnt[MRG_OVER]) { if (threadIdx.x == 0) ent[0] = -1; return; }
  if (kGreedy) det_scan_emit(p.mask, a.wpr, p.cnt[MRG_N], p.sbox, p.sprob, p.ssrc, a.pack.dets + 5 * slot, a.pack.ids + slot, ent, dyn_lds);
  else det_color_emit(p.mask, a.wpr, p.cnt[MRG_N], p.sbox, p.sprob, p.ssrc, a.pack.dets + 5 * slot, a.pack.ids + slot, ent, dyn_lds);
}
__global__ __launch_bounds__(256) void det_merge_scan_emit_kernel(DetMergeArgs a) {
  extern __shared__ __attribute__((aligned(16))) u64 dyn_lds[];
  det_merge_emit<true>(a, dyn_lds);
}
__global__ __launch_bounds__(256) void det_merge_color_emit_kernel(DetMergeArgs a) {
  extern __shared__ __attribute__((aligned(16))) u64 dyn_lds[];
  det_merge_emit<false>(a, dyn_lds);
}

// -- merge, lists of more than kMaxK slots: one list at a time on the tiled path (det_tiled_nms), this its key kernel
// keys[0 .. P): the list's keys, then zero padding; cnt[DC_N] = the list's length (0 when it overflowed), the tiled path's state cleared
__global__ __launch_bounds__(256) void det_merge_keys_big_kernel(const int* __restrict__ lcnt, const float* __restrict__ prob, int cap,
                                                                 u64* __restrict__ keys, int P, int* __restrict__ cnt) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int wanted = lcnt[CAND_WANTED];
  const int n = (lcnt[CAND_OVER] || wanted > cap || wanted < 0) ? 0 : wanted;
  static_assert(DC_BIG_WORDS == 2, "the state words cleared below");
  if (i == 0) { cnt[DC_N] = n; cnt[DC_BIG] = 0; cnt[DC_BIG + 1] = 0; }
  if (i < P) keys[i] = i < n ? det_key(prob[i], i) : 0ull;
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
          const double o = det_overlap<false>(A, as_a, xe_a, ye_a, B);      // (the bit matrix's overlap, the union form)
          if (!(o >= a.thr)) continue;      // (no overlap, or a NaN ratio: no vote)
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
}  // namespace

using namespace mscnn;

namespace mscnn_dev {
void det_merge_sort_launch(const DetMergeArgs& a, int ns, hipStream_t st) { det_merge_sort_kernel<<<ns, kSortThreads, 0, st>>>(a); }
void det_merge_keys_big_launch(const int* lcnt, const float* prob, int cap, u64* keys, int P, int* cnt, hipStream_t st) {
  det_merge_keys_big_kernel<<<cdiv(P, 256), 256, 0, st>>>(lcnt, prob, cap, keys, P, cnt);
}
}  // namespace mscnn_dev

extern "C" size_t mscnn_detections_merge_workspace_bytes(int num_segments, int cand_cap) {
  if (!cand_shape_ok(num_segments, cand_cap)) return 0;
  if (cand_cap > kMaxK) return mscnn_detections_workspace_bytes(cand_cap);      // one list at a time
  return det_slices_bytes(num_segments, cand_cap, false);
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
  const DetPack pack = det_pack_of(pack_dev, S, S * cand_cap);
  if (!big) {
    DetMergeArgs a = {};
    a.cand_cap = cand_cap; a.wpr = (cand_cap + 63) / 64; a.num_segs = S;
    a.cand = static_cast<char*>(cand); a.ws = static_cast<char*>(workspace);
    a.seg_stride_box = det_slice_box_bytes(cand_cap, false); a.seg_stride_mask = det_slice_mask_bytes(cand_cap);
    a.pack = pack;
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
  // one list at a time on the tiled path; the list's length comes from its device count
  const DetCand c = det_cand_of(static_cast<char*>(cand), S, cand_cap);
  const DetTiled w = det_tiled_of(workspace, cand_cap);
  for (int s = 0; s < S; ++s) {
    const size_t list = (size_t)s * (size_t)cand_cap;
    det_merge_keys_big_kernel<<<cdiv(w.P, 256), 256, 0, st>>>(c.cnt + CAND_WORDS * (size_t)s, c.prob + list, cand_cap, w.keys, w.P, w.cnt);
    MSCNN_POST_LAUNCH();
    if (int rc = det_tiled_nms(workspace, cand_cap, c.box + list, c.prob + list, c.tag + list, nms_overlap[s], pack.dets + 5 * list,
                               pack.ids + list, pack.hdr + MSCNN_MULTI_PACK_WORDS * (size_t)(1 + s), st))
      return rc;
  }
  det_merge_table_big_kernel<<<cdiv(S, 256), 256, 0, st>>>(c.cnt, S, cand_cap, pack.hdr);
  MSCNN_POST_LAUNCH();
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
  const DetPack pack = det_pack_of(pack_dev, S, S * cand_cap);
  DetVoteArgs a;
  a.num_segs = S; a.cand_cap = cand_cap; a.thr = vote->thr;
  a.cand = const_cast<char*>(static_cast<const char*>(cand));
  a.hdr = pack.hdr;
  a.dets = pack.dets;
  det_merge_vote_kernel<<<kVoteBlocks, kVoteThreads, 0, as_stream(stream)>>>(a);
  MSCNN_POST_LAUNCH();
  return MSCNN_OK;
}
