// Soft-NMS over the merged candidates (mscnn_detections_merge_soft_fwd): serial in picks, parallel in candidates.  One workgroup of
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
#include "det_device.h"

namespace {
using namespace mscnn_dev;

constexpr int kSoftThreads = 1024, kSoftWaves = kSoftThreads / 64, kSoftPer = 4, kSoftRegs = kSoftThreads * kSoftPer;
constexpr int kSoftNone = 0x7fffffff;      // the slot of "nothing live": loses every tie
struct DetSoftArgs {
  int cand_cap, num_segs, s0, method, max_out;
  double sigma, score_thr;
  char* cand; char* ws; size_t seg_stride;
  DetPack pack;
  double overlap[kSegsPerLaunch];
};
struct SoftBest { double s; int slot; };
struct SoftPick { double s; int slot; int pad; DetBox box; };

__host__ __device__ __forceinline__ size_t det_soft_seg_bytes(int cap) {      // the streaming path's scores and live flags of one list
  return cap > kSoftRegs ? det_al((size_t)cap * sizeof(double)) + det_al((size_t)cap) : 0;
}
// a NaN ranks below every number
__device__ __forceinline__ double soft_rank(double s) { return s != s ? -__builtin_inf() : s; }
// the total order of the argmax: the larger score, then the lower slot
__device__ __forceinline__ bool soft_better(double sa, int ia, double sb, int ib) { return sa > sb || (sa == sb && ia < ib); }
__device__ __forceinline__ void soft_take(SoftBest& b, double s, int slot) {
  s = soft_rank(s);
  if (soft_better(s, slot, b.s, b.slot)) { b.s = s; b.slot = slot; }
}
// the score of candidate B after the pick of box A (step 5 of the contract, one statement per operation: det_overlap<false>'s, written
// out here -- through the helper this kernel, at 126 VGPRs, gained instructions in every decay of a pick)
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
  int* ent = a.pack.hdr + MSCNN_MULTI_PACK_WORDS * (size_t)(1 + s);
  if (s == 0 && tid == 0) { a.pack.hdr[0] = a.num_segs; a.pack.hdr[1] = a.cand_cap; a.pack.hdr[2] = a.num_segs * a.cand_cap; a.pack.hdr[3] = 0; }
  if (tid == 0) { ent[1] = wanted; ent[2] = (int)list; ent[3] = 0; }
  if (over || wanted > a.cand_cap) { if (tid == 0) ent[0] = -1; return; }      // the list overflowed: nothing else of it is written
  const int n = wanted < 0 ? 0 : wanted;
  const DetBox* box = c.box + list;
  const float* prob = c.prob + list;
  const int* tag = c.tag + list;
  double* dets = a.pack.dets + 5 * list;
  int* ids = a.pack.ids + list;
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
    unsigned char* ws_live = reinterpret_cast<unsigned char*>(w + det_al((size_t)a.cand_cap * sizeof(double)));
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
}  // namespace

using namespace mscnn;

extern "C" size_t mscnn_detections_merge_soft_workspace_bytes(int num_segments, int cand_cap) {
  if (!cand_shape_ok(num_segments, cand_cap)) return 0;
  // (the launches of a call follow each other on the stream and share the per-segment areas; a list in registers needs none)
  const size_t segs = (size_t)(num_segments < kSegsPerLaunch ? num_segments : kSegsPerLaunch);
  const size_t need = segs * det_soft_seg_bytes(cand_cap);
  return need > det_al(1) ? need : det_al(1);
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
  DetSoftArgs a = {};
  a.cand_cap = cand_cap; a.num_segs = S; a.method = soft->method; a.max_out = soft->max_out;
  a.sigma = soft->sigma; a.score_thr = soft->score_thr;
  a.cand = static_cast<char*>(cand); a.ws = static_cast<char*>(workspace); a.seg_stride = det_soft_seg_bytes(cand_cap);
  a.pack = det_pack_of(pack_dev, S, S * cand_cap);
  for (int s0 = 0; s0 < S; s0 += kSegsPerLaunch) {
    const int ns = S - s0 < kSegsPerLaunch ? S - s0 : kSegsPerLaunch;
    a.s0 = s0;
    for (int j = 0; j < ns; ++j) a.overlap[j] = nms_overlap[s0 + j];
    det_merge_soft_kernel<<<ns, kSoftThreads, 0, as_stream(stream)>>>(a);
    MSCNN_POST_LAUNCH();
  }
  return MSCNN_OK;
}
