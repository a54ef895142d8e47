// Seq-NMS over the candidate lists of a clip's frames (mscnn_detections_merge_seq_fwd; Han, Khorrami, Paine et al., "Seq-NMS for Video
// Object Detection", 2016): link the boxes of neighbouring frames by overlap, take the chain of boxes with the largest score sum, give
// its boxes the chain's score, suppress what they overlap in their own frames, again.  Segment s = t * K + k is the list of frame t,
// slot k; chain k is the segments k, K + k, ...; chains never interact.  A list is sorted by the merge's own sort
// (det_merge_sort_launch, or key kernel + big_sort_desc + det_tiled_gather above kMaxK slots, as det_wbf.hip); det_seq_enter_kernel
// copies the candidates that ENTER (the leading ones with s >= score_thr, at most top_k <= kSeqThreads) into the op's own state, where
// all frames stay side by side.  det_seq_link_kernel then builds the link bits of every frame pair in one parallel launch: row j of
// frame t = one bit per box of frame t - 1, a wave per row, a ballot per word.  ONE workgroup of kSeqThreads then owns a chain
// (det_seq_chain_kernel): thread j is box j of the frame at hand.  An iteration: the DP over the frames in ascending order (the live
// masks of all frames and the V / len of the previous frame sit in LDS, prev of all frames in the workspace, one barrier per frame),
// each thread's best end box over its frames, a butterfly over the wave and the waves' bests through LDS to the same winner in every
// thread; thread 0 walks the path back through prev; every frame of the path then outputs its path box and clears the live bits the
// box overlaps -- the overlap recomputed, a wave rewrites its own live word from a ballot.  The DP always restarts at frame 0: the
// result does not depend on it, and a restart at the removed path's first frame would need every thread's best over the frames before.
// Every maximum is taken under a total order (seq_better; the DP's strict > over ascending i), every sum is one add per frame in
// frame order: no reduction shape, grid size or timing decides a bit.  Every loop bound and every value that guards a barrier is a
// kernel argument, a device count read into LDS before the first barrier, or the winner read out of LDS, the same in all threads;
// an iteration kills at least its end box, so the loop runs at most sum m_t times and carries that bound; no atomics on global
// memory, nothing spins, no workgroup waits on another.  det_seq_emit_kernel (a workgroup per segment) ranks a segment's output
// boxes and writes the table entry and the rows.
#include "det_device.h"
#include "nms_large.h"

namespace {
using namespace mscnn_dev;

constexpr int kSeqThreads = 1024, kSeqWaves = kSeqThreads / 64;      // a thread is a box of the frame at hand: top_k <= kSeqThreads
constexpr int kSeqWords = kSeqThreads / 64;                         // live words per frame in LDS
constexpr int kSeqMaxFrames = 256;                                  // kSeqMaxFrames * kSeqWords live words = 32 KB of LDS
constexpr int kSeqLinkRows = 4;                                     // rows (waves) per workgroup of the link kernel
constexpr int kSeqGridY = 32768;                                    // segments per link launch (gridDim.y)
constexpr int kSeqMaxCap = 1 << 30;                                 // big_sort_desc's power of two is an int

// the op's state behind the sort's area: per segment m (the boxes that entered) and the nms overlap, per entered box the box, s, tag,
// score' and sequence id (-1: not output), prev of the last DP, and its link row (wk words over the frame before)
struct SeqState { int* m; double* thr; DetBox* box; double* s; int* tag; double* oscore; int* oq; int* prev; u64* link; };
__host__ __device__ __forceinline__ size_t seq_state_bytes(size_t S, int top_k) {
  const size_t n = S * (size_t)top_k, wk = (size_t)((top_k + 63) / 64);
  return det_al(S * sizeof(int)) + det_al(S * sizeof(double)) + det_al(n * sizeof(DetBox)) + 2 * det_al(n * sizeof(double)) +
         3 * det_al(n * sizeof(int)) + det_al(n * wk * sizeof(u64));
}
__host__ __device__ __forceinline__ SeqState seq_state_of(char* p, size_t S, int top_k) {
  const size_t n = S * (size_t)top_k;
  SeqState w;
  w.m = reinterpret_cast<int*>(p); p += det_al(S * sizeof(int));
  w.thr = reinterpret_cast<double*>(p); p += det_al(S * sizeof(double));
  w.box = reinterpret_cast<DetBox*>(p); p += det_al(n * sizeof(DetBox));
  w.s = reinterpret_cast<double*>(p); p += det_al(n * sizeof(double));
  w.oscore = reinterpret_cast<double*>(p); p += det_al(n * sizeof(double));
  w.tag = reinterpret_cast<int*>(p); p += det_al(n * sizeof(int));
  w.oq = reinterpret_cast<int*>(p); p += det_al(n * sizeof(int));
  w.prev = reinterpret_cast<int*>(p); p += det_al(n * sizeof(int));
  w.link = reinterpret_cast<u64*>(p);
  return w;
}
inline size_t seq_big_sort_bytes(int cap) {      // [cnt][keys][sbox][sprob][ssrc] of the list at hand (det_wbf.hip's layout)
  return 256 + det_al((size_t)big_sort_pow2(cap) * sizeof(u64)) + det_al((size_t)cap * sizeof(DetBox)) + det_al((size_t)cap * sizeof(double)) +
         det_al((size_t)cap * sizeof(int));
}
inline size_t seq_small_sort_bytes(int S, int cap) {
  return det_al((size_t)S * kSliceWords * sizeof(int)) + (size_t)S * det_slice_box_bytes(cap, false);
}

// -- step 1: the candidates that enter, out of the sorted list
struct SeqEnterArgs {
  int cand_cap, num_segs, s0, top_k, big;
  double score_thr;
  char* ws; size_t seg_stride_box;      // lists of at most kMaxK slots: the merge's slices (det_slice_of, no bit matrix behind them)
  const int* bcnt; const DetBox* bsbox; const double* bsprob; const int* bssrc;      // a longer list: the one at hand, sorted
  char* state;
  double overlap[kSegsPerLaunch];
};

__global__ __launch_bounds__(kSeqThreads) void det_seq_enter_kernel(SeqEnterArgs a) {
  __shared__ int first;
  const int j = blockIdx.x, s = a.s0 + j, tid = threadIdx.x;
  int n; const DetBox* sbox; const double* sprob; const int* ssrc;
  if (a.big) {
    n = a.bcnt[DC_N]; sbox = a.bsbox; sprob = a.bsprob; ssrc = a.bssrc;
  } else {
    const DetSlice p = det_slice_of<false>(a.ws, a.num_segs, a.cand_cap, a.seg_stride_box, 0, s);
    n = p.cnt[MRG_N]; sbox = p.sbox; sprob = p.sprob; ssrc = p.ssrc;
  }
  n = n < 0 ? 0 : (n > a.cand_cap ? a.cand_cap : n);      // (0: an empty or an overflowed list)
  const int lim = n < a.top_k ? n : a.top_k;
  if (tid == 0) first = lim;
  __syncthreads();
  const double sc = tid < lim ? sprob[tid] : 0.0;
  if (tid < lim && !(sc >= a.score_thr)) atomicMin(&first, tid);      // (LDS; a NaN fails.  The minimum: its order decides nothing)
  __syncthreads();
  const int m = first;
  const SeqState w = seq_state_of(a.state, (size_t)a.num_segs, a.top_k);
  if (tid == 0) { w.m[s] = m; w.thr[s] = a.overlap[j]; }
  if (tid >= m) return;
  const size_t e = (size_t)s * (size_t)a.top_k + (size_t)tid;
  w.box[e] = sbox[tid]; w.s[e] = sc; w.tag[e] = ssrc[tid]; w.oq[e] = -1;
}

// -- step 2: the link bits.  Segments [s0, s0 + gridDim.y), s0 >= K: row j of frame t over the boxes of frame t - 1
struct SeqLinkArgs { int num_segs, num_slots, top_k, wk, s0; double link_thr; char* state; };

__global__ __launch_bounds__(64 * kSeqLinkRows) void det_seq_link_kernel(SeqLinkArgs a) {
  const int s = a.s0 + (int)blockIdx.y, lane = threadIdx.x & 63;
  const int j = (int)blockIdx.x * kSeqLinkRows + (int)(threadIdx.x >> 6);
  const SeqState w = seq_state_of(a.state, (size_t)a.num_segs, a.top_k);
  const int mj = w.m[s], mp = w.m[s - a.num_slots];      // (<= top_k each)
  if (j >= mj) return;
  const size_t e = (size_t)s * (size_t)a.top_k + (size_t)j, pe = (size_t)(s - a.num_slots) * (size_t)a.top_k;
  const DetBox B = w.box[e];
  u64* row = w.link + e * (size_t)a.wk;
  for (int q = 0; q * 64 < mp; ++q) {      // (q < wk: mp <= top_k)
    const int i = q * 64 + lane;
    bool on = false;
    if (i < mp) {
      const DetBox A = w.box[pe + i];
      on = det_overlap<false>(A, A.w * A.h, A.x + A.w, A.y + A.h, B) > a.link_thr;      // (no overlap, or a NaN ratio: no link)
    }
    const u64 bits = __ballot(on);
    if (lane == 0) row[q] = bits;
  }
}

// -- steps 3 to 10: one workgroup per chain
struct SeqBest { double v; int t, j, len; };      // t < 0: none
// the total order of the end box: the larger V, then the lower t, then the lower j; "none" loses to everything
__device__ __forceinline__ bool seq_better(const SeqBest& a, const SeqBest& b) {
  if (a.t < 0) return false;
  if (b.t < 0) return true;
  return a.v > b.v || (a.v == b.v && (a.t < b.t || (a.t == b.t && a.j < b.j)));
}

struct SeqChainArgs { int num_frames, num_slots, top_k, wk, rescore; char* state; };

__global__ __launch_bounds__(kSeqThreads) void det_seq_chain_kernel(SeqChainArgs a) {
  __shared__ u64 live[kSeqMaxFrames][kSeqWords];
  __shared__ double vb[2][kSeqThreads];
  __shared__ int lb[2][kSeqThreads];
  __shared__ int mt[kSeqMaxFrames], pathj[kSeqMaxFrames];
  __shared__ SeqBest red[kSeqWaves];
  __shared__ int s_first;
  __shared__ double s_score;
  const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = a.num_frames, K = a.num_slots;
  const SeqState w = seq_state_of(a.state, (size_t)T * (size_t)K, a.top_k);
  for (int t = tid; t < T; t += kSeqThreads) {
    int m = w.m[(size_t)t * K + k];
    m = m < 0 ? 0 : (m > a.top_k ? a.top_k : m);
    mt[t] = m;
  }
  __syncthreads();
  int total = 0;
  for (int t = 0; t < T; ++t) total += mt[t];
  for (int i = tid; i < T * kSeqWords; i += kSeqThreads) {      // step 3: all entered boxes are live
    const int rem = mt[i / kSeqWords] - 64 * (i % kSeqWords);
    live[i / kSeqWords][i % kSeqWords] = rem >= 64 ? ~0ull : (rem > 0 ? (1ull << rem) - 1ull : 0ull);
  }
  __syncthreads();
  for (int q = 0; q < total; ++q) {      // (an iteration kills at least its end box)
    // step 4: the DP, frames ascending; this thread's best end box over its frames (strict >: the lower t among equal V)
    SeqBest b = {0.0, -1, tid, 0};
    for (int t = 0; t < T; ++t) {
      const size_t e = ((size_t)t * K + k) * (size_t)a.top_k + (size_t)tid;
      if (tid < mt[t] && ((live[t][wave] >> lane) & 1ull)) {
        const double s = w.s[e];
        double pv = 0.0;
        int p = -1;
        if (t > 0) {
          const int wp = (mt[t - 1] + 63) >> 6;
          const u64* row = w.link + e * (size_t)a.wk;
          const double* vp = vb[(t - 1) & 1];
          for (int c = 0; c < wp; ++c) {
            u64 bits = row[c] & live[t - 1][c];
            while (bits) {      // ascending i, strict >: the lowest i among equal V
              const int i = c * 64 + __ffsll((unsigned long long)bits) - 1;
              bits &= bits - 1ull;
              const double v = vp[i];
              if (p < 0 || v > pv) { pv = v; p = i; }
            }
          }
        }
        const double V = p < 0 ? s : pv + s;
        const int len = p < 0 ? 1 : lb[(t - 1) & 1][p] + 1;
        w.prev[e] = p;
        vb[t & 1][tid] = V; lb[t & 1][tid] = len;
        if (b.t < 0 || V > b.v) { b.v = V; b.t = t; b.len = len; }
      }
      __syncthreads();      // (frame t's V / len are written; every thread is done with the buffer frame t + 1 writes)
    }
    // step 5: the end of the best path, the same in every thread
    for (int m = 1; m <= 32; m <<= 1) {
      SeqBest o;
      o.v = __shfl_xor(b.v, m); o.t = __shfl_xor(b.t, m); o.j = __shfl_xor(b.j, m); o.len = __shfl_xor(b.len, m);
      if (seq_better(o, b)) b = o;
    }
    if (lane == 0) red[wave] = b;
    __syncthreads();
    SeqBest E = red[0];
    for (int c = 1; c < kSeqWaves; ++c) {
      const SeqBest o = red[c];
      if (seq_better(o, E)) E = o;
    }
    if (E.t < 0) break;      // no live box is left (the same in every thread)
    // the path, back through prev (written before the barriers above), and step 6
    if (tid == 0) {
      int t = E.t, j = E.j;
      double mx = 0.0;
      for (int c = 0; c < E.len && t >= 0 && j >= 0; ++c) {
        pathj[t] = j;
        const size_t e = ((size_t)t * K + k) * (size_t)a.top_k + (size_t)j;
        const double s = w.s[e];
        if (c == 0 || s > mx) mx = s;
        j = w.prev[e];
        --t;
      }
      s_first = t + 1;
      s_score = a.rescore == MSCNN_SEQ_NMS_AVG ? E.v / (double)E.len : mx;
    }
    __syncthreads();
    // steps 7 and 8, frame by frame of the path: a wave rewrites its own live word
    const int t0 = s_first;
    const double score = s_score;
    for (int t = t0; t <= E.t; ++t) {
      const int js = pathj[t];
      const size_t base = ((size_t)t * K + k) * (size_t)a.top_k;
      bool keep = tid < mt[t] && ((live[t][wave] >> lane) & 1ull);
      if (keep) {
        if (tid == js) {
          w.oscore[base + tid] = score; w.oq[base + tid] = q;
          keep = false;
        } else {
          const DetBox A = w.box[base + js], B = w.box[base + tid];
          if (det_overlap<false>(A, A.w * A.h, A.x + A.w, A.y + A.h, B) > w.thr[(size_t)t * K + k]) keep = false;
        }
      }
      const u64 bits = __ballot(keep);
      if (lane == 0) live[t][wave] = bits;
    }
    __syncthreads();      // (the next DP reads every wave's live words; red, pathj, s_first and s_score are free again)
  }
}

// -- step 11: one workgroup per segment: table entry, rank, rows
struct SeqEmitArgs { int num_segs, cand_cap, top_k, max_out; char* cand; char* state; DetPack pack; int* seq; };

__global__ __launch_bounds__(kSeqThreads) void det_seq_emit_kernel(SeqEmitArgs a) {
  __shared__ double sc[kSeqThreads];
  __shared__ int on[kSeqThreads];
  __shared__ int total;
  const int s = blockIdx.x, tid = threadIdx.x;
  const DetCand cd = det_cand_of(a.cand, a.num_segs, a.cand_cap);      // (read only)
  const int wanted = cd.cnt[CAND_WORDS * (size_t)s + CAND_WANTED], over = cd.cnt[CAND_WORDS * (size_t)s + CAND_OVER];
  const size_t list = (size_t)s * (size_t)a.cand_cap;
  int* ent = a.pack.hdr + MSCNN_MULTI_PACK_WORDS * (size_t)(1 + s);
  if (s == 0 && tid == 0) { a.pack.hdr[0] = a.num_segs; a.pack.hdr[1] = a.cand_cap; a.pack.hdr[2] = a.num_segs * a.cand_cap; a.pack.hdr[3] = 0; }
  if (tid == 0) { ent[1] = wanted; ent[2] = (int)list; ent[3] = 0; }
  if (over || wanted > a.cand_cap) { if (tid == 0) ent[0] = -1; return; }      // the list overflowed: nothing else of it is written
  const SeqState w = seq_state_of(a.state, (size_t)a.num_segs, a.top_k);
  int m = w.m[s];
  m = m < 0 ? 0 : (m > a.top_k ? a.top_k : m);
  const size_t e = (size_t)s * (size_t)a.top_k + (size_t)tid;
  const int q = tid < m ? w.oq[e] : -1;
  const double my = q >= 0 ? w.oscore[e] : 0.0;
  sc[tid] = my; on[tid] = q >= 0 ? 1 : 0;
  if (tid == 0) total = 0;
  __syncthreads();
  if (q >= 0) atomicAdd(&total, 1);      // (LDS; a count: its order decides nothing)
  __syncthreads();
  const int C = total;
  const int count = (a.max_out > 0 && C > a.max_out) ? a.max_out : C;
  if (tid == 0) ent[0] = count;
  if (q < 0) return;
  int before = 0;      // the larger score', then the lower sorted position
  for (int i = 0; i < m; ++i) before += (on[i] && (sc[i] > my || (sc[i] == my && i < tid))) ? 1 : 0;
  if (before >= count) return;
  const DetBox B = w.box[e];
  double* d = a.pack.dets + 5 * (list + (size_t)before);
  d[0] = B.x; d[1] = B.y; d[2] = B.w; d[3] = B.h; d[4] = my;
  a.pack.ids[list + (size_t)before] = w.tag[e];
  if (a.seq) a.seq[list + (size_t)before] = q;
}

inline bool seq_shape_ok(int T, int K, int cap, int top_k) {
  if (T < 1 || T > kSeqMaxFrames || K < 1 || cap < 1 || cap > kSeqMaxCap || top_k < 1 || top_k > kSeqThreads) return false;
  const long S = (long)T * (long)K;
  return S <= 0x7fffffffL && cand_shape_ok((int)S, cap);
}
}  // namespace

using namespace mscnn;

extern "C" size_t mscnn_detections_merge_seq_workspace_bytes(int num_frames, int num_slots, int cand_cap, int top_k) {
  if (!seq_shape_ok(num_frames, num_slots, cand_cap, top_k)) return 0;
  const int S = num_frames * num_slots;
  const size_t sort = cand_cap > kMaxK ? seq_big_sort_bytes(cand_cap) : seq_small_sort_bytes(S, cand_cap);      // (a long list is sorted alone)
  return sort + seq_state_bytes((size_t)S, top_k);
}

extern "C" int mscnn_detections_merge_seq_fwd(const double* nms_overlap, const mscnn_seq_nms_params* sq, int num_frames, int num_slots,
                                              void* cand, int cand_cap, void* pack_dev, int* seq_dev, void* workspace,
                                              size_t workspace_bytes, void* stream) {
  MSCNN_REQUIRE(nms_overlap && sq && cand && pack_dev && workspace, "detections_merge_seq: null pointer");
  const int T = num_frames, K = num_slots;
  MSCNN_REQUIRE(T >= 1 && T <= kSeqMaxFrames, "detections_merge_seq: num_frames %d is outside [1, %d]", T, kSeqMaxFrames);
  MSCNN_REQUIRE(K >= 1, "detections_merge_seq: num_slots %d", K);
  MSCNN_REQUIRE(cand_cap >= 1, "detections_merge_seq: cand_cap %d", cand_cap);
  MSCNN_REQUIRE((long)T * (long)K <= 0x7fffffffL && cand_shape_ok(T * K, cand_cap),
                "detections_merge_seq: %d frames x %d slots x %d candidate slots is past 2^31 - 1", T, K, cand_cap);
  MSCNN_REQUIRE(cand_cap <= kSeqMaxCap, "detections_merge_seq: cand_cap %d is past the sort's 2^30 keys", cand_cap);
  MSCNN_REQUIRE(sq->top_k >= 1 && sq->top_k <= kSeqThreads, "detections_merge_seq: top_k %d is outside [1, %d]", sq->top_k, kSeqThreads);
  MSCNN_REQUIRE(sq->link_thr > 0 && sq->link_thr < 1, "detections_merge_seq: link_thr %g is not inside (0, 1)", sq->link_thr);      // (NaN included)
  MSCNN_REQUIRE(sq->score_thr >= 0 && sq->score_thr < __builtin_inf(), "detections_merge_seq: score_thr %g is not a finite value >= 0",
                sq->score_thr);
  MSCNN_REQUIRE(sq->rescore == MSCNN_SEQ_NMS_AVG || sq->rescore == MSCNN_SEQ_NMS_MAX,
                "detections_merge_seq: rescore %d is neither %d (avg) nor %d (max)", sq->rescore, MSCNN_SEQ_NMS_AVG, MSCNN_SEQ_NMS_MAX);
  MSCNN_REQUIRE(sq->max_out >= 0, "detections_merge_seq: max_out %d", sq->max_out);
  const int S = T * K;
  for (int s = 0; s < S; ++s) MSCNN_REQUIRE(!(nms_overlap[s] != nms_overlap[s]), "detections_merge_seq: segment %d: nms_overlap is NaN", s);
  MSCNN_REQUIRE_ALIGNED(cand, 16, "detections_merge_seq: cand");
  MSCNN_REQUIRE_ALIGNED(workspace, 16, "detections_merge_seq: workspace");
  MSCNN_REQUIRE_ALIGNED(pack_dev, 16, "detections_merge_seq: pack_dev");
  MSCNN_REQUIRE_ALIGNED(seq_dev, 4, "detections_merge_seq: seq_dev");
  const size_t need = mscnn_detections_merge_seq_workspace_bytes(T, K, cand_cap, sq->top_k);
  if (workspace_bytes < need) {
    set_error("detections_merge_seq: workspace %zu < %zu", workspace_bytes, need);
    return MSCNN_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  const bool big = cand_cap > kMaxK;
  const int top_k = sq->top_k, wk = (top_k + 63) / 64;
  char* ws = static_cast<char*>(workspace);
  char* state = ws + (big ? seq_big_sort_bytes(cand_cap) : seq_small_sort_bytes(S, cand_cap));
  const DetPack pack = det_pack_of(pack_dev, S, S * cand_cap);
  SeqEnterArgs en = {};
  en.cand_cap = cand_cap; en.num_segs = S; en.top_k = top_k; en.big = big ? 1 : 0; en.score_thr = sq->score_thr; en.state = state;
  if (!big) {
    DetMergeArgs m = {};      // the merge's sort on its own slices; no bit matrix follows them (stride 0, never touched)
    m.cand_cap = cand_cap; m.wpr = 0; m.num_segs = S; m.cand = static_cast<char*>(cand); m.ws = ws;
    m.seg_stride_box = det_slice_box_bytes(cand_cap, false); m.seg_stride_mask = 0; m.pack = pack;
    en.ws = ws; en.seg_stride_box = m.seg_stride_box;
    for (int s0 = 0; s0 < S; s0 += kSegsPerLaunch) {
      const int ns = S - s0 < kSegsPerLaunch ? S - s0 : kSegsPerLaunch;
      m.s0 = s0; en.s0 = s0;
      for (int j = 0; j < ns; ++j) en.overlap[j] = nms_overlap[s0 + j];
      det_merge_sort_launch(m, ns, st);
      MSCNN_POST_LAUNCH();
      det_seq_enter_kernel<<<ns, kSeqThreads, 0, st>>>(en);
      MSCNN_POST_LAUNCH();
    }
  } else {
    // list after list: the tiled path's key kernel, sort and gather; the list's length is its device count
    const DetCand c = det_cand_of(static_cast<char*>(cand), S, cand_cap);
    const int P = big_sort_pow2(cand_cap);
    int* bcnt = reinterpret_cast<int*>(ws);
    char* p = ws + 256;
    u64* keys = reinterpret_cast<u64*>(p); p += det_al((size_t)P * sizeof(u64));
    DetBox* sbox = reinterpret_cast<DetBox*>(p); p += det_al((size_t)cand_cap * sizeof(DetBox));
    double* sprob = reinterpret_cast<double*>(p); p += det_al((size_t)cand_cap * sizeof(double));
    int* ssrc = reinterpret_cast<int*>(p);
    en.bcnt = bcnt; en.bsbox = sbox; en.bsprob = sprob; en.bssrc = ssrc;
    for (int s = 0; s < S; ++s) {
      const size_t list = (size_t)s * (size_t)cand_cap;
      det_merge_keys_big_launch(c.cnt + CAND_WORDS * (size_t)s, c.prob + list, cand_cap, keys, P, bcnt, st);
      MSCNN_POST_LAUNCH();
      MSCNN_HIP_TRY(big_sort_desc(keys, P, st));
      det_tiled_gather(keys, c.box + list, c.prob + list, c.tag + list, sbox, sprob, ssrc, bcnt, cand_cap, st);
      MSCNN_POST_LAUNCH();
      en.s0 = s; en.overlap[0] = nms_overlap[s];
      det_seq_enter_kernel<<<1, kSeqThreads, 0, st>>>(en);
      MSCNN_POST_LAUNCH();
    }
  }
  SeqLinkArgs ln = {S, K, top_k, wk, 0, sq->link_thr, state};
  for (int s0 = K; s0 < S; s0 += kSeqGridY) {      // (frame 0 has no frame before it)
    const int ns = S - s0 < kSeqGridY ? S - s0 : kSeqGridY;
    ln.s0 = s0;
    det_seq_link_kernel<<<dim3(cdiv(top_k, kSeqLinkRows), ns), 64 * kSeqLinkRows, 0, st>>>(ln);
    MSCNN_POST_LAUNCH();
  }
  const SeqChainArgs ch = {T, K, top_k, wk, sq->rescore, state};
  det_seq_chain_kernel<<<K, kSeqThreads, 0, st>>>(ch);
  MSCNN_POST_LAUNCH();
  const SeqEmitArgs em = {S, cand_cap, top_k, sq->max_out, static_cast<char*>(cand), state, pack, seq_dev};
  det_seq_emit_kernel<<<S, kSeqThreads, 0, st>>>(em);
  MSCNN_POST_LAUNCH();
  return MSCNN_OK;
}
