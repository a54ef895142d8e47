// A streaming multi-object tracker behind the final stage (mscnn_tracks_update_fwd): BYTE's two association passes (Zhang et al.,
// "ByteTrack: Multi-Object Tracking by Associating Every Detection Box", 2022) over the multi pack's rows, a small table of tracks per
// slot kept in device memory from call to call, a persistent track id for every detection row.  Two things have the paper's way on
// request beside the tracker's own: the motion is a constant-velocity prediction of the box centre (the paper's Kalman filter: the KF
// instantiations of the kernel, mscnn_tracks_update_kalman_fwd), and the matching is greedy by descending overlap under a total order
// (larger r, then the lower track, then the lower detection; the optimal assignment: the OPT instantiations,
// mscnn_tracks_update_assign_fwd, track_pass_optimal below).
// The frames of a call may belong to several streams (cameras): mscnn_tracks_update_streams_fwd gives every (stream, slot) a table of
// its own and one workgroup, side by side in one launch; the map frame -> stream travels by value in the kernel arguments.
// ONE workgroup of kTrackThreads owns a slot for the whole call and loops over the call's frames; thread i is track i AND detection i
// of the frame at hand (hence max_tracks <= 1024 and the 1024 detections that enter).  A thread keeps its track's record and its
// detection's row in registers: the table is loaded once per call and stored once.
// The greedy walk runs as rounds of "match every mutually-best pair": because the order on pairs is total, a pair that is the best
// remaining pair of both its track and its detection is picked by the walk before any other pair that uses either of them, so the
// rounds give the walk's matching (tests/track_witness.py does both and compares).  A round: the free tracks' boxes go to LDS and every
// free detection scans them for its best track (strict > over ascending i: the lower i among equal r); the free detections' boxes go
// to the SAME 32 KB of LDS and every free track scans them for its best detection; a track whose best detection names it back is
// matched.  A thread scans again only when the partner it found is no longer free: the free sets only shrink, so a best partner that
// is still free is still the best.  r(i, j) is det_overlap<false>(track box, detection) from both sides: the same statements, the same
// bits.  The loop carries its own bound, min(tracks, detections) rounds, and ends earlier at the first round that matches nothing.
// Every loop bound and every value that guards a barrier is a kernel argument, a word of the pack or the state every thread reads
// alike, a count every thread sums alike out of LDS, or the round's "any" word read behind a barrier.  No atomics at all, nothing
// spins, no workgroup waits on another.  The compaction's places come from ballots and popcounts, the records move through the LDS box buffer field by
// field.  All arithmetic is double, one statement per operation (-ffp-contract=off): bit-exact against tests/track_witness.py.
#include "det_device.h"

namespace {
using namespace mscnn_dev;

constexpr int kTrackThreads = 1024, kTrackWaves = kTrackThreads / 64;      // a thread is a track and a detection
constexpr int kTrackStreams = 256;      // streams of a call, and frames of a call with more than one stream: stream_of rides in the arguments

struct TrackArgs {
  mscnn_track_params p;
  int num_frames, num_slots, cap, max_tracks;
  size_t dets_at, slot_bytes, records_at;      // the pack's rows; the state's slot stride and the records behind a slot's header
  const char* pack;
  const char* state_in; char* state_out;
  int* ids;
  int num_streams;
  unsigned short stream_of[kTrackStreams];      // frame t's stream; read only when num_streams > 1 (then num_frames <= kTrackStreams)
};
// the arguments of the Kalman instantiation (mscnn_tracks_update_kalman_fwd): the same, then the filter's setting and its two tables
// The products that do not depend on a track are made once, on the host, in the same double arithmetic (one rounding each): in
// the kernel they would be hoisted out of the frame loop into vector registers the kernel does not have.
struct TrackKalmanArgs : TrackArgs {
  double sp, sv;              // std_position, std_velocity
  double sp2, sv10;           // 2 * std_position, 10 * std_velocity (step 8')
  double a2, b2, m2;          // std_aspect, std_aspect_velocity, std_aspect_measure, each times itself
  int freeze_lost_height;
  const mscnn_track_kalman_record* filter_in;
  mscnn_track_kalman_record* filter_out;
};
using KalmanRecord = mscnn_track_kalman_record;

// Where a thread's filter record lives.  The track record, the detection and the association's scans fill the 128 VGPRs a lane of a
// 1024-thread workgroup may have; 40 more for the filter record spill.  So the mean and its velocity (x, v: 16 VGPRs) stay in
// registers and the 12 covariance numbers (p, q, r per component) lie in LDS between their uses, a column per thread: 96 KB beside the
// 58 KB of the association, 154 of gfx950's 160 KB per workgroup -- in the Kalman instantiation only.  A column is touched by its own
// thread only, except at the compaction, which reads, waits at a barrier, and writes.
constexpr int kKalmanCov = 12;      // p[4], q[4], r[4]
template <bool KF>
__device__ __forceinline__ double* kalman_cov() {
  if constexpr (KF) {
    __shared__ double cov[kKalmanCov * kTrackThreads];
    return cov + threadIdx.x;
  } else {
    return nullptr;
  }
}
// number j of p / q / r (0 / 1 / 2) of component c in a thread's column
__device__ __forceinline__ int kalman_at(int j, int c) { return (4 * j + c) * kTrackThreads; }

// step 3': one component of the prediction (sp2 = sigp * sigp, sv2 = sigv * sigv)
__device__ __forceinline__ void kalman_predict1(double& x, double v, double* cov, int c, double sp2, double sv2) {
  const double p = cov[kalman_at(0, c)], q = cov[kalman_at(1, c)], r = cov[kalman_at(2, c)];
  x = x + v;
  const double t0 = p + q, t1 = q + r, t2 = t0 + t1;
  cov[kalman_at(0, c)] = t2 + sp2; cov[kalman_at(1, c)] = t1; cov[kalman_at(2, c)] = r + sv2;
}
// step 6': one component of the update with the measurement z (sm2 = sigm * sigm)
__device__ __forceinline__ void kalman_update1(double& x, double& v, double* cov, int c, double z, double sm2) {
  const double p = cov[kalman_at(0, c)], q = cov[kalman_at(1, c)], r = cov[kalman_at(2, c)];
  const double s = p + sm2, kx = p / s, kv = q / s, y = z - x;
  const double ax = kx * y, av = kv * y, dr = kv * q, dp = kx * p, dq = kx * q;
  x = x + ax; v = v + av;
  cov[kalman_at(2, c)] = r - dr; cov[kalman_at(0, c)] = p - dp; cov[kalman_at(1, c)] = q - dq;
}
// the box of a filter's mean: (cx, cy, a, h) -> {x, y, w, h}
__device__ __forceinline__ void kalman_box(const double* x, double* box) {
  const double w = x[2] * x[3], hw = w / 2, hh = x[3] / 2;
  box[0] = x[0] - hw; box[1] = x[1] - hh; box[2] = w; box[3] = x[3];
}

// the places of the set flags among the workgroup's threads, and their number (every thread calls it; two barriers)
__device__ __forceinline__ int track_rank(bool on, int* wsum, int* total_out, int tid = threadIdx.x) {
  const int lane = tid & 63, wave = tid >> 6;
  const u64 bits = __ballot(on);
  if (lane == 0) wsum[wave] = __popcll(bits);
  __syncthreads();
  int before = 0, total = 0;
  for (int c = 0; c < kTrackWaves; ++c) {
    const int v = wsum[c];
    before += c < wave ? v : 0;
    total += v;
  }
  __syncthreads();      // (wsum is free again)
  *total_out = total;
  return before + __popcll(bits & ((1ull << lane) - 1ull));
}

// One association pass.  tact: this thread's track takes part (and is free); dact: this thread's detection does.  tbox / dbox: the
// thread's own track box and detection.  n tracks, m detections.  Returns through tmatch (the detection matched to this thread's
// track) and dmatch (the track matched to this thread's detection); both stay as they were for the unmatched.
__device__ __forceinline__ void track_pass(bool tact, bool dact, const DetBox& tbox, const DetBox& dbox, int n, int m, double thr,
                                           DetBox* buf, int* best_d, int* dmatch_l, unsigned char* tfree, unsigned char* dfree, int* any,
                                           int* tmatch, int* dmatch) {
  const int tid = threadIdx.x;
  tfree[tid] = tact ? 1 : 0;
  dfree[tid] = dact ? 1 : 0;
  best_d[tid] = -1;
  dmatch_l[tid] = -1;
  int my_bt = -2, my_bd = -2;      // the best track of my detection / the best detection of my track (-2: not scanned, -1: none)
  const int rounds = n < m ? n : m;
  for (int q = 0; q < rounds; ++q) {
    if (tid == 0) *any = 0;
    if (tid < n) buf[tid] = tbox;
    __syncthreads();      // (the flags of the last round and the track boxes are written)
    if (dact && dfree[tid] && (my_bt == -2 || (my_bt >= 0 && !tfree[my_bt]))) {
      double br = 0.0;
      my_bt = -1;
      for (int i = 0; i < n; ++i) {
        if (!tfree[i]) continue;
        const DetBox A = buf[i];
        const double r = det_overlap<false>(A, A.w * A.h, A.x + A.w, A.y + A.h, dbox);
        if (r > thr && (my_bt < 0 || r > br)) { br = r; my_bt = i; }      // (no overlap or a NaN r: no pair)
      }
      best_d[tid] = my_bt;
    }
    __syncthreads();      // (every scan of the track boxes is done)
    if (tid < m) buf[tid] = dbox;
    __syncthreads();
    if (tact && tfree[tid] && (my_bd == -2 || (my_bd >= 0 && !dfree[my_bd]))) {
      const double as_a = tbox.w * tbox.h, xe_a = tbox.x + tbox.w, ye_a = tbox.y + tbox.h;
      double br = 0.0;
      my_bd = -1;
      for (int j = 0; j < m; ++j) {
        if (!dfree[j]) continue;
        const double r = det_overlap<false>(tbox, as_a, xe_a, ye_a, buf[j]);
        if (r > thr && (my_bd < 0 || r > br)) { br = r; my_bd = j; }
      }
    }
    __syncthreads();      // (every scan has read the flags: they may change now)
    if (tact && tfree[tid] && my_bd >= 0 && best_d[my_bd] == tid) {      // mutually best: the walk takes this pair first
      tfree[tid] = 0; dfree[my_bd] = 0; dmatch_l[my_bd] = tid;
      *tmatch = my_bd;
      *any = 1;
    }
    __syncthreads();
    if (!*any) break;      // (the same word in every thread; it is written again only behind the next barrier)
    __syncthreads();
  }
  __syncthreads();
  if (dact && dmatch_l[tid] >= 0) *dmatch = dmatch_l[tid];
  __syncthreads();      // (the arrays are free again)
}

// ---- the optimal form of a pass (steps 4'' and 5'' of mscnn_tracks_update_assign_fwd): a maximum-weight matching over the eligible
// pairs by shortest augmenting paths with potentials, all in int64.  Thread i is row i (its track) AND real column i (its detection) AND
// row i's private dummy column.  In registers: minv and used of the real column, "reached" of the dummy.  A dummy is reached by its own
// row only, so its v stays 0, it is never used before the step that ends a search, its way / p are its row's column, and its minv is
// -u[row] from the step that reaches it on: it starts as that, and every later step takes delta from it and adds delta to u[row],
// whose column is used by then (or whose row is x).  In LDS, all but 4 KB in arrays the greedy pass owns and a pass leaves free: every
// track box for the whole pass (buf), u (sbuf's 8 KB), way and p of the real columns (best_d, dmatch_l), the column of every row (xa),
// "takes part" and "has an eligible pair" per row (dfree, tfree), v of the real columns as two words (xb and 4 KB of its own: the
// Kalman instantiation has no two registers left for it).  New beside that: the 16 wave minima of a step, 128 bytes.  A step: one det_overlap per thread, one workgroup-wide minimum of the key minv * 2048 + column
// (the lower column among equal minv; a dummy's column is 1024 + its row, so real columns come first), two barriers.  i0, j0, delta, j1
// and "j1 is free" are read out of LDS behind a barrier by every thread alike; the walk back is one thread's, behind a barrier.
constexpr long long kAssignInf = 0x7fffffffffffffffLL;
__device__ __forceinline__ long long track_q(double x) { return (long long)floor(x * 1073741824.0); }      // floor(x * 2^30): exact
template <bool OPT>
__device__ __forceinline__ long long* assign_red() {
  if constexpr (OPT) {
    __shared__ long long red[kTrackWaves];
    return red;
  } else {
    return nullptr;
  }
}
template <bool OPT>
__device__ __forceinline__ int* assign_vhi() {
  if constexpr (OPT) {
    __shared__ int vhi[kTrackThreads];
    return vhi;
  } else {
    return nullptr;
  }
}
// Returns the pass's steps.  tmatch / dmatch as track_pass.  fill: buf gets the track boxes (pass 1); pass 2 finds them there.
template <bool fill>
__device__ __forceinline__ int track_pass_optimal(bool tact, bool dact, const DetBox& tbox, const DetBox& dbox, int n, int m, double thr,
                                                  DetBox* buf, long long* u, int* way, int* prow, int* rcol, unsigned char* has,
                                                  unsigned char* act, long long* red, int* vlo, int* vhi, int* tmatch, int* dmatch) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  has[tid] = 0;
  act[tid] = tact ? 1 : 0;
  if constexpr (fill) { if (tid < n) buf[tid] = tbox; }
  u[tid] = 0; way[tid] = -1; prow[tid] = -1; rcol[tid] = -1; vlo[tid] = 0; vhi[tid] = 0;
  __syncthreads();
  if (dact) {      // the rows that have an eligible pair: the others stay unmatched and cost no step
    for (int i = 0; i < n; ++i) {
      if (!act[i]) continue;
      const DetBox A = buf[i];
      const double r = det_overlap<false>(A, A.w * A.h, A.x + A.w, A.y + A.h, dbox);
      if (r > thr) has[i] = 1;      // (every writer stores the same byte)
    }
  }
  __syncthreads();
  const long long qthr = track_q(thr);
  const int bound = (n < m ? n : m) + 1;      // (>= min(a, b) + 1: every step of a search uses a new assigned column or ends)
  int steps = 0;
  for (int x = 0; x < n; ++x) {
    if (!has[x]) continue;      // (LDS behind a barrier: every thread alike)
    long long minv_r = kAssignInf;
    bool used_r = false, reached = false, ended = false;
    int i0 = x, j0 = -1, j1 = -1;
    for (int s = 0; s < bound; ++s) {
      steps += steps < 0x7fffffff ? 1 : 0;
      const long long ui = u[i0];
      if (dact && !used_r) {
        const DetBox A = buf[i0];
        const double r = det_overlap<false>(A, A.w * A.h, A.x + A.w, A.y + A.h, dbox);
        if (r > thr) {
          const long long v_r = (long long)(((unsigned long long)(unsigned)vhi[tid] << 32) | (unsigned)vlo[tid]);
          const long long cur = -(track_q(r) - qthr + 1) - ui - v_r;
          if (cur < minv_r) { minv_r = cur; way[tid] = j0; }
        }
      }
      if (tid == i0) reached = true;      // (its dummy: cost 0, v 0, way j0, minv = -u[tid] from here on)
      long long key = (!used_r && minv_r != kAssignInf) ? minv_r * 2048 + tid : kAssignInf;
      const long long kd = reached ? -u[tid] * 2048 + (kTrackThreads + tid) : kAssignInf;
      key = kd < key ? kd : key;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) { const long long other = __shfl_xor(key, o); key = other < key ? other : key; }
      if (lane == 0) red[wave] = key;
      __syncthreads();
#pragma unroll
      for (int c = 0; c < kTrackWaves; ++c) { const long long other = red[c]; key = other < key ? other : key; }
      const long long delta = key >> 11;      // (x's own dummy has a finite minv from the first step on: the key is never kAssignInf)
      j1 = (int)(key & 2047);
      const int nx = j1 < kTrackThreads ? prow[j1] : -1;      // (a dummy is free whenever it is reached)
      if (tid == x) u[x] += delta;
      if (used_r) {      // (the rows of the used columns are distinct, and none is x)
        u[prow[tid]] += delta;
        const long long v_r = (long long)(((unsigned long long)(unsigned)vhi[tid] << 32) | (unsigned)vlo[tid]) - delta;
        vlo[tid] = (int)(unsigned)v_r; vhi[tid] = (int)(v_r >> 32);
      } else if (minv_r != kAssignInf) {
        minv_r -= delta;
      }
      if (tid == j1) used_r = true;
      __syncthreads();      // (u is written, red is free again)
      j0 = j1;
      if (nx < 0) { ended = true; break; }
      i0 = nx;
    }
    if (ended && tid == 0) {      // augment back along way
      int j = j1;
      for (int g = 0; g < bound && j >= 0; ++g) {
        int jp;
        if (j >= kTrackThreads) { const int row = j - kTrackThreads; jp = row == x ? -1 : rcol[row]; }
        else jp = way[j];
        // (a column inside a path is a real one and has a row; the masks keep the indices inside the arrays whatever happens)
        const int row = (jp < 0 ? x : prow[jp & (kTrackThreads - 1)]) & (kTrackThreads - 1);
        if (j < kTrackThreads) prow[j] = row;
        rcol[row] = j;
        j = jp;
      }
    }
    __syncthreads();
  }
  if (dact && prow[tid] >= 0) *dmatch = prow[tid];
  if (tact) { const int c = rcol[tid]; if (c >= 0 && c < kTrackThreads) *tmatch = c; }
  __syncthreads();      // (the arrays are free again)
  return steps;
}

// KF false: the motions none / linear of mscnn_tracks_update_fwd / _streams_fwd, Args = TrackArgs.  KF true: steps 3', 6', 8', 9' of
// mscnn_tracks_update_kalman_fwd, Args = TrackKalmanArgs; the association passes, the ids and the compaction of the track records are
// the same statements.  A thread's filter record F is touched by its own thread only, except at the compaction.
// OPT false: the greedy walk (track_pass), header word 5 is written 0.  OPT true: the optimal assignment (track_pass_optimal) in
// both passes, header word 5 is the table's running total of steps.
template <bool KF, bool OPT, class Args>
__global__ __launch_bounds__(kTrackThreads) void det_track_kernel(Args a) {
  __shared__ DetBox buf[kTrackThreads];
  __shared__ double sbuf[kTrackThreads];
  __shared__ int best_d[kTrackThreads], dmatch_l[kTrackThreads], xa[kTrackThreads], xb[kTrackThreads];
  __shared__ unsigned char tfree[kTrackThreads], dfree[kTrackThreads];
  __shared__ int wsum[kTrackWaves];
  __shared__ int any;
  const int k = blockIdx.x, tid = threadIdx.x;
  const int K = a.num_slots;
  const int strm = blockIdx.y;                                    // this workgroup's stream
  const size_t tab = (size_t)strm * (size_t)K + (size_t)k;      // its table: slot strm * K + k of the state
  const int* hdr = reinterpret_cast<const int*>(a.pack);
  const double* rows = reinterpret_cast<const double*>(a.pack + a.dets_at);
  const bool linear = a.p.motion == MSCNN_TRACK_MOTION_LINEAR;

  // the slot's header and this thread's record
  const int* hin = reinterpret_cast<const int*>(a.state_in + a.slot_bytes * tab);
  int n = hin[MSCNN_TRACKS_N], next_id = hin[MSCNN_TRACKS_NEXT_ID], frame = hin[MSCNN_TRACKS_FRAME];
  int dropped = hin[MSCNN_TRACKS_DROPPED], skipped = hin[MSCNN_TRACKS_SKIPPED];
  int steps = 0;
  long long* const red = assign_red<OPT>();
  int* const vhi = assign_vhi<OPT>();
  if constexpr (OPT) { steps = hin[MSCNN_TRACKS_STEPS]; steps = steps < 0 ? 0 : steps; }
  n = n < 0 ? 0 : (n > a.max_tracks ? a.max_tracks : n);      // (a table that was never reset: nothing past max_tracks is touched)
  mscnn_track_record R = {};
  if (tid < n) R = reinterpret_cast<const mscnn_track_record*>(a.state_in + a.slot_bytes * tab + a.records_at)[tid];
  double fx[4] = {0.0, 0.0, 0.0, 0.0}, fv[4] = {0.0, 0.0, 0.0, 0.0};      // the filter's mean and velocity; its covariance: cov
  double* const cov = kalman_cov<KF>();
  const int frame_in = frame;
  if constexpr (KF) {
    R.vel[0] = 0.0; R.vel[1] = 0.0;      // (not kept in registers: see where the record is stored)
    if (tid < n) {
      const KalmanRecord* f = a.filter_in + tab * (size_t)a.max_tracks + (size_t)tid;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        fx[c] = f->x[c]; fv[c] = f->v[c];
        cov[kalman_at(0, c)] = f->p[c]; cov[kalman_at(1, c)] = f->q[c]; cov[kalman_at(2, c)] = f->r[c];
      }
    }
  }

  for (int t = 0; t < a.num_frames; ++t) {
    if (a.num_streams > 1 && (int)a.stream_of[t] != strm) continue;      // another stream's frame (arguments and blockIdx only: every thread alike)
    frame += 1;                                                                               // step 1
    // step 2: the segment's entry and this thread's detection
    const int s = t * K + k;
    const int* ent = hdr + MSCNN_MULTI_PACK_WORDS * (size_t)(1 + s);
    const int count = ent[0];
    long long off = ent[2];
    if (K >= 2) {      // an image's slots share row0 (mscnn_detections_multi_fwd); a merged list has a row offset of its own
      const int* e0 = hdr + MSCNN_MULTI_PACK_WORDS * (size_t)(1 + t * K);
      if (e0[2] == e0[MSCNN_MULTI_PACK_WORDS + 2]) off = (long long)mscnn_multi_pack_slot(K, ent[2], k, ent[1]);
    }
    const bool fits = count >= 0 && off >= 0 && off + (long long)count <= (long long)a.cap;      // (else: an empty frame, no id written)
    const int m = !fits ? 0 : (count < kTrackThreads ? count : kTrackThreads);
    if (fits) skipped += count - m;
    DetBox B = {0.0, 0.0, 0.0, 0.0};
    double sc = 0.0;
    int cls = 0;      // 1: in H, 2: in L
    if (tid < m) {
      const double* d = rows + 5 * ((size_t)off + (size_t)tid);
      B.x = d[0]; B.y = d[1]; B.w = d[2]; B.h = d[3]; sc = d[4];
      cls = sc >= a.p.high_thr ? 1 : (sc >= a.p.low_thr ? 2 : 0);      // (a NaN score is in neither set)
    }
    const bool have = tid < n;
    if constexpr (KF) {                                                                       // step 3'
      if (have) {
        if (a.freeze_lost_height != 0 && R.misses > 0) fv[3] = 0.0;
        const double h = fx[3], e = a.sp * h, g = a.sv * h, e2 = e * e, g2 = g * g;
        kalman_predict1(fx[0], fv[0], cov, 0, e2, g2);
        kalman_predict1(fx[1], fv[1], cov, 1, e2, g2);
        kalman_predict1(fx[2], fv[2], cov, 2, a.a2, a.b2);
        kalman_predict1(fx[3], fv[3], cov, 3, e2, g2);
        kalman_box(fx, R.box);      // (vel = {v[0], v[1]}: made where the record is stored)
      }
    } else {
      if (linear && have) { R.box[0] += R.vel[0]; R.box[1] += R.vel[1]; }                     // step 3
    }
    const DetBox T = {R.box[0], R.box[1], R.box[2], R.box[3]};
    int tmatch = -1, dmatch = -1;
    if constexpr (OPT) {                                                                      // steps 4'' and 5''
      long long* const u = reinterpret_cast<long long*>(sbuf);
      int k = track_pass_optimal<true>(have, cls == 1, T, B, n, m, a.p.match_thr, buf, u, best_d, dmatch_l, xa, tfree, dfree, red, xb, vhi, &tmatch, &dmatch);
      steps = k > 0x7fffffff - steps ? 0x7fffffff : steps + k;
      if (a.p.low_thr < a.p.high_thr) {
        k = track_pass_optimal<false>(have && tmatch < 0 && R.misses == 0 && R.confirmed != 0, cls == 2, T, B, n, m, a.p.match_thr_low, buf, u,
                                      best_d, dmatch_l, xa, tfree, dfree, red, xb, vhi, &tmatch, &dmatch);
        steps = k > 0x7fffffff - steps ? 0x7fffffff : steps + k;
      }
      // The track's box comes back out of buf, where it lay for both passes: so it holds no registers while the searches run (the
      // Kalman instantiation has none to spare), and the second pass needs no copy of it either.
      if (have) { const DetBox D = buf[tid]; R.box[0] = D.x; R.box[1] = D.y; R.box[2] = D.w; R.box[3] = D.h; }
      __syncthreads();      // (buf is free again)
    } else {
      track_pass(have, cls == 1, T, B, n, m, a.p.match_thr, buf, best_d, dmatch_l, tfree, dfree, &any, &tmatch, &dmatch);      // step 4
      if (a.p.low_thr < a.p.high_thr)                                                         // step 5 (L is empty otherwise)
        track_pass(have && tmatch < 0 && R.misses == 0 && R.confirmed != 0, cls == 2, T, B, n, m, a.p.match_thr_low, buf, best_d,
                   dmatch_l, tfree, dfree, &any, &tmatch, &dmatch);
    }
    // Behind the optimal passes the thread's index passes through an empty asm statement: what the rest of the frame derives from it
    // (LDS and global addresses, lane masks) is then made here and holds no registers while the searches run.  tq == tid.
    int tq = tid;
    if constexpr (OPT) { asm volatile("" : "+v"(tq)); __builtin_assume(tq >= 0 && tq < kTrackThreads); }
    // steps 6 and 7: a matched detection hands its row to its track through LDS
    if (dmatch >= 0) { buf[dmatch] = B; sbuf[dmatch] = sc; }
    __syncthreads();
    bool alive = false;
    if (have) {
      if (tmatch >= 0) {
        const DetBox D = buf[tq];
        if (linear) {
          const double g = (double)(R.misses + 1);
          const double hw = D.w / 2, hx = D.x + hw, ow = R.obs[2] / 2, ox = R.obs[0] + ow;
          const double dx = (hx - ox) / g;
          const double hh = D.h / 2, hy = D.y + hh, oh = R.obs[3] / 2, oy = R.obs[1] + oh;
          const double dy = (hy - oy) / g;
          if (R.hits == 1) {
            R.vel[0] = dx; R.vel[1] = dy;
          } else {
            const double ex = dx - R.vel[0], gx = a.p.vel_gain * ex;
            R.vel[0] = R.vel[0] + gx;
            const double ey = dy - R.vel[1], gy = a.p.vel_gain * ey;
            R.vel[1] = R.vel[1] + gy;
          }
        }
        if constexpr (KF) {                                                                   // step 6'
          const double hw = D.w / 2, zx = D.x + hw, hh = D.h / 2, zy = D.y + hh, za = D.w / D.h;
          const double h = fx[3], e = a.sp * h, e2 = e * e;
          kalman_update1(fx[0], fv[0], cov, 0, zx, e2);
          kalman_update1(fx[1], fv[1], cov, 1, zy, e2);
          kalman_update1(fx[2], fv[2], cov, 2, za, a.m2);
          kalman_update1(fx[3], fv[3], cov, 3, D.h, e2);
          kalman_box(fx, R.box);
        } else {
          R.box[0] = D.x; R.box[1] = D.y; R.box[2] = D.w; R.box[3] = D.h;
        }
        R.obs[0] = D.x; R.obs[1] = D.y; R.obs[2] = D.w; R.obs[3] = D.h;
        R.score = sbuf[tq];
        R.hits += 1; R.misses = 0;
        if (R.hits >= a.p.min_hits) R.confirmed |= 1;
        alive = true;
      } else {
        R.misses += 1;
        alive = R.confirmed != 0 && R.misses <= a.p.max_age;
      }
      xa[tq] = R.confirmed != 0 ? R.id : 0;      // what a detection matched to this track is given
    }
    const bool born = cls == 1 && dmatch < 0 && sc >= a.p.new_thr;                            // step 8
    // step 9: the survivors in their old order, then the births in ascending j; the first max_tracks
    int nsurv = 0, nborn = 0;
    const int ps = track_rank(alive, wsum, &nsurv, tq);      // (its barriers also publish xa)
    const int pb = track_rank(born, wsum, &nborn, tq);
    const int room = a.max_tracks - nsurv;               // (>= 0: nsurv <= n <= max_tracks)
    const int kept = nborn < room ? nborn : room;
    const bool born_kept = born && pb < kept;
    // step 10
    if (tq < m) {
      int id = 0;
      if (dmatch >= 0) id = xa[dmatch];
      else if (born_kept && a.p.min_hits <= 1) id = next_id + pb;
      a.ids[(size_t)off + (size_t)tq] = id;
    }
    if (fits)
      for (int j = kTrackThreads + tq; j < count; j += kTrackThreads) a.ids[(size_t)off + (size_t)j] = 0;      // (never entered)
    __syncthreads();      // (xa is free again)
    if (nsurv != n || kept > 0) {      // the records move to their new places, field by field through LDS
      const int pd = nsurv + pb;
      if (alive) { buf[ps] = DetBox{R.box[0], R.box[1], R.box[2], R.box[3]}; sbuf[ps] = R.score; xa[ps] = R.id; xb[ps] = R.hits; }
      if (born_kept) { buf[pd] = B; sbuf[pd] = sc; xa[pd] = next_id + pb; xb[pd] = 1; }
      __syncthreads();
      const int n2 = nsurv + kept;
      mscnn_track_record N = {};
      if (tq < n2) { const DetBox D = buf[tq]; N.box[0] = D.x; N.box[1] = D.y; N.box[2] = D.w; N.box[3] = D.h; N.score = sbuf[tq]; N.id = xa[tq]; N.hits = xb[tq]; }
      __syncthreads();
      if (alive) { buf[ps] = DetBox{R.obs[0], R.obs[1], R.obs[2], R.obs[3]}; if constexpr (!KF) sbuf[ps] = R.vel[0]; xa[ps] = R.misses; xb[ps] = R.confirmed; }
      if (born_kept) { buf[pd] = B; if constexpr (!KF) sbuf[pd] = 0.0; xa[pd] = 0; xb[pd] = a.p.min_hits <= 1 ? 1 : 0; }
      __syncthreads();
      if (tq < n2) { const DetBox D = buf[tq]; N.obs[0] = D.x; N.obs[1] = D.y; N.obs[2] = D.w; N.obs[3] = D.h; if constexpr (!KF) N.vel[0] = sbuf[tq]; N.misses = xa[tq]; N.confirmed = xb[tq]; }
      __syncthreads();
      if constexpr (!KF) {      // (the filter's tracks: vel is the filter's v[0], v[1], which moves below)
        if (alive) sbuf[ps] = R.vel[1];
        if (born_kept) sbuf[pd] = 0.0;
        __syncthreads();
        if (tq < n2) N.vel[1] = sbuf[tq];
        __syncthreads();
      }
      R = N;
      if constexpr (KF) {      // step 9': the filter records move with their tracks, a component (x, v, p, q | r) at a time through
        // the box buffer: a thread reads its own column in front of the barrier and writes its own column behind it, so a column
        // stays its thread's.  Step 8': a birth's record is made where it is sent.
        const double hw = B.w / 2, hh = B.h / 2;
        const double z[4] = {B.x + hw, B.y + hh, B.w / B.h, B.h};
        const double e = a.sp2 * B.h, e2 = e * e, g = a.sv10 * B.h, g2 = g * g;
        double a2 = a.a2, b2 = a.b2;
        if constexpr (OPT) asm volatile("" : "+s"(a2), "+s"(b2));      // (as tq: no copy of them in vector registers during the searches)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if (alive) { buf[ps] = DetBox{fx[c], fv[c], cov[kalman_at(0, c)], cov[kalman_at(1, c)]}; sbuf[ps] = cov[kalman_at(2, c)]; }
          if (born_kept) { buf[pd] = DetBox{z[c], 0.0, c == 2 ? a2 : e2, 0.0}; sbuf[pd] = c == 2 ? b2 : g2; }
          __syncthreads();
          if (tq < n2) {
            const DetBox D = buf[tq];
            fx[c] = D.x; fv[c] = D.y; cov[kalman_at(0, c)] = D.w; cov[kalman_at(1, c)] = D.h; cov[kalman_at(2, c)] = sbuf[tq];
          }
          __syncthreads();
        }
      }
      n = n2;
    }
    dropped += nborn - kept;
    next_id += kept;
  }

  char* so = a.state_out + a.slot_bytes * tab;
  if (tid == 0) {
    int* h = reinterpret_cast<int*>(so);
    h[MSCNN_TRACKS_N] = n; h[MSCNN_TRACKS_NEXT_ID] = next_id; h[MSCNN_TRACKS_FRAME] = frame; h[MSCNN_TRACKS_DROPPED] = dropped;
    h[MSCNN_TRACKS_SKIPPED] = skipped; h[MSCNN_TRACKS_STEPS] = OPT ? steps : 0; h[6] = 0; h[7] = 0;
  }
  if constexpr (KF) {      // vel = {v[0], v[1]} behind every step 3', 6' and 8'; a table that was not stepped keeps the vel it came with
    if (tid < n) {
      if (frame != frame_in) {
        R.vel[0] = fv[0]; R.vel[1] = fv[1];
      } else {
        const mscnn_track_record* in = reinterpret_cast<const mscnn_track_record*>(a.state_in + a.slot_bytes * tab + a.records_at) + tid;
        R.vel[0] = in->vel[0]; R.vel[1] = in->vel[1];      // (in place: this thread's own record, which it writes below)
      }
    }
  }
  if (tid < n) reinterpret_cast<mscnn_track_record*>(so + a.records_at)[tid] = R;      // (records at index >= n stay as they were)
  if constexpr (KF) {
    if (tid < n) {      // (records at index >= n stay as they were)
      KalmanRecord* f = a.filter_out + tab * (size_t)a.max_tracks + (size_t)tid;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        f->x[c] = fx[c]; f->v[c] = fv[c];
        f->p[c] = cov[kalman_at(0, c)]; f->q[c] = cov[kalman_at(1, c)]; f->r[c] = cov[kalman_at(2, c)];
      }
    }
  }
}

__global__ void det_track_reset_kernel(char* state, size_t slot_bytes, int first_slot, int num_slots) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= num_slots) return;
  int* h = reinterpret_cast<int*>(state + slot_bytes * ((size_t)first_slot + (size_t)k));
  h[MSCNN_TRACKS_N] = 0; h[MSCNN_TRACKS_NEXT_ID] = 1; h[MSCNN_TRACKS_FRAME] = 0; h[MSCNN_TRACKS_DROPPED] = 0; h[MSCNN_TRACKS_SKIPPED] = 0;
  h[5] = 0; h[6] = 0; h[7] = 0;
}

inline bool track_shape_ok(int K, int max_tracks) { return K >= 1 && max_tracks >= 1 && max_tracks <= kTrackThreads; }
}  // namespace

using namespace mscnn;

extern "C" size_t mscnn_tracks_state_bytes(int num_slots, int max_tracks) {
  if (!track_shape_ok(num_slots, max_tracks)) return 0;
  return mscnn_tracks_state_layout_of(num_slots, max_tracks).total;
}

extern "C" int mscnn_tracks_state_reset(void* state, int num_slots, int max_tracks, void* stream) {
  MSCNN_REQUIRE(state, "tracks_state_reset: null state");
  MSCNN_REQUIRE(num_slots >= 1, "tracks_state_reset: num_slots %d", num_slots);
  MSCNN_REQUIRE(max_tracks >= 1 && max_tracks <= kTrackThreads, "tracks_state_reset: max_tracks %d is outside [1, %d]", max_tracks, kTrackThreads);
  MSCNN_REQUIRE_ALIGNED(state, 16, "tracks_state_reset: state");
  const mscnn_tracks_state_layout L = mscnn_tracks_state_layout_of(num_slots, max_tracks);
  det_track_reset_kernel<<<cdiv(num_slots, 256), 256, 0, as_stream(stream)>>>(static_cast<char*>(state), L.slot, 0, num_slots);
  MSCNN_POST_LAUNCH();
  return MSCNN_OK;
}

extern "C" int mscnn_tracks_state_reset_slots(void* state, int num_slots_total, int max_tracks, int first_slot, int count, void* stream) {
  MSCNN_REQUIRE(state, "tracks_state_reset_slots: null state");
  MSCNN_REQUIRE(num_slots_total >= 1, "tracks_state_reset_slots: num_slots_total %d", num_slots_total);
  MSCNN_REQUIRE(max_tracks >= 1 && max_tracks <= kTrackThreads, "tracks_state_reset_slots: max_tracks %d is outside [1, %d]", max_tracks, kTrackThreads);
  MSCNN_REQUIRE(first_slot >= 0 && count >= 0 && (long)first_slot + (long)count <= (long)num_slots_total,
                "tracks_state_reset_slots: slots [%d, %d + %d) are outside [0, %d]", first_slot, first_slot, count, num_slots_total);
  MSCNN_REQUIRE_ALIGNED(state, 16, "tracks_state_reset_slots: state");
  if (count == 0) return MSCNN_OK;
  const mscnn_tracks_state_layout L = mscnn_tracks_state_layout_of(num_slots_total, max_tracks);
  det_track_reset_kernel<<<cdiv(count, 256), 256, 0, as_stream(stream)>>>(static_cast<char*>(state), L.slot, first_slot, count);
  MSCNN_POST_LAUNCH();
  return MSCNN_OK;
}

// All entry points: `op` names the one that was called in a refusal.  with_map false: one stream, no map (mscnn_tracks_update_fwd).
// kc: the call of mscnn_tracks_update_kalman_fwd (the Kalman instantiation, its filter tables and setting), null for the other two.
// assign: MSCNN_TRACK_ASSIGN_GREEDY for the three ops that have no say in it; map_optional: a null stream_of passes with one stream.
static int tracks_update_any(const char* op, bool with_map, const mscnn_track_params* p, int num_frames, int num_slots, int num_streams, const int* stream_of,
                             const void* pack_dev, int cap, const void* state_in, void* state_out, int max_tracks, int* track_ids_dev,
                             void* stream, const mscnn_tracks_kalman_call* kc = nullptr, int assign = MSCNN_TRACK_ASSIGN_GREEDY,
                             bool map_optional = false) {
  MSCNN_REQUIRE(p && pack_dev && state_in && state_out && track_ids_dev, "%s: null pointer", op);
  MSCNN_REQUIRE(assign == MSCNN_TRACK_ASSIGN_GREEDY || assign == MSCNN_TRACK_ASSIGN_OPTIMAL, "%s: assign %d is neither %d (greedy) nor %d (optimal)", op,
                assign, MSCNN_TRACK_ASSIGN_GREEDY, MSCNN_TRACK_ASSIGN_OPTIMAL);
  if (kc) {
    MSCNN_REQUIRE(kc->filter, "%s: null filter", op);
    MSCNN_REQUIRE(kc->filter_in, "%s: null filter_in", op);
    MSCNN_REQUIRE(kc->filter_out, "%s: null filter_out", op);
  }
  const int T = num_frames, K = num_slots;
  MSCNN_REQUIRE(T >= 1, "%s: num_frames %d", op, T);
  MSCNN_REQUIRE(K >= 1, "%s: num_slots %d", op, K);
  MSCNN_REQUIRE(cap >= 1, "%s: cap %d", op, cap);
  const int N = num_streams;
  if (with_map) {
    MSCNN_REQUIRE(stream_of || ((kc || map_optional) && N == 1), "%s: null stream_of", op);
    MSCNN_REQUIRE(N >= 1 && N <= kTrackStreams, "%s: num_streams %d is outside [1, %d]", op, N, kTrackStreams);
    MSCNN_REQUIRE(N == 1 || T <= kTrackStreams, "%s: num_frames %d is above %d with %d streams (the map rides in the kernel's arguments)", op, T,
                  kTrackStreams, N);
    for (int t = 0; stream_of && t < T; ++t)
      MSCNN_REQUIRE(stream_of[t] >= 0 && stream_of[t] < N, "%s: stream_of[%d] = %d is outside [0, %d)", op, t, stream_of[t], N);
    MSCNN_REQUIRE((long)N * (long)K <= 0x7fffffffL, "%s: %d streams x %d slots is past 2^31 - 1", op, N, K);
  }
  MSCNN_REQUIRE((long)T * (long)K <= 0x7fffffffL && (long)T * (long)K * (long)cap <= 0x7fffffffL,
                "%s: %d frames x %d slots x %d pack rows is past 2^31 - 1", op, T, K, cap);
  MSCNN_REQUIRE(max_tracks >= 1 && max_tracks <= kTrackThreads, "%s: max_tracks %d is outside [1, %d]", op, max_tracks, kTrackThreads);
  MSCNN_REQUIRE(!(p->high_thr != p->high_thr), "%s: high_thr is NaN", op);
  MSCNN_REQUIRE(!(p->low_thr != p->low_thr), "%s: low_thr is NaN", op);
  MSCNN_REQUIRE(!(p->new_thr != p->new_thr), "%s: new_thr is NaN", op);
  MSCNN_REQUIRE(p->match_thr >= 0 && p->match_thr < 1, "%s: match_thr %g is not inside [0, 1)", op, p->match_thr);      // (NaN included)
  MSCNN_REQUIRE(p->match_thr_low >= 0 && p->match_thr_low < 1, "%s: match_thr_low %g is not inside [0, 1)", op, p->match_thr_low);
  MSCNN_REQUIRE(p->low_thr <= p->high_thr, "%s: low_thr %g is above high_thr %g", op, p->low_thr, p->high_thr);
  MSCNN_REQUIRE(p->new_thr >= p->high_thr, "%s: new_thr %g is below high_thr %g", op, p->new_thr, p->high_thr);
  if (kc) {      // (vel_gain is not read)
    MSCNN_REQUIRE(p->motion == MSCNN_TRACK_MOTION_NONE, "%s: motion %d is not %d (none): the filter is the motion", op, p->motion,
                  MSCNN_TRACK_MOTION_NONE);
    const mscnn_track_kalman_params& f = *kc->filter;
    const double stds[5] = {f.std_position, f.std_velocity, f.std_aspect, f.std_aspect_velocity, f.std_aspect_measure};
    const char* const names[5] = {"std_position", "std_velocity", "std_aspect", "std_aspect_velocity", "std_aspect_measure"};
    for (int i = 0; i < 5; ++i)      // (NaN included)
      MSCNN_REQUIRE(stds[i] > 0 && stds[i] <= 1.7976931348623157e308, "%s: %s %g is not a finite number above 0", op, names[i], stds[i]);
  } else {
    MSCNN_REQUIRE(p->vel_gain > 0 && p->vel_gain <= 1, "%s: vel_gain %g is not inside (0, 1]", op, p->vel_gain);
    MSCNN_REQUIRE(p->motion == MSCNN_TRACK_MOTION_NONE || p->motion == MSCNN_TRACK_MOTION_LINEAR,
                  "%s: motion %d is neither %d (none) nor %d (linear)", op, p->motion, MSCNN_TRACK_MOTION_NONE, MSCNN_TRACK_MOTION_LINEAR);
  }
  MSCNN_REQUIRE(p->max_age >= 0, "%s: max_age %d", op, p->max_age);
  MSCNN_REQUIRE(p->min_hits >= 1, "%s: min_hits %d", op, p->min_hits);
  MSCNN_REQUIRE(reinterpret_cast<uintptr_t>(pack_dev) % 16 == 0, "%s: pack_dev must be 16-byte aligned", op);
  MSCNN_REQUIRE(reinterpret_cast<uintptr_t>(state_in) % 16 == 0, "%s: state_in must be 16-byte aligned", op);
  MSCNN_REQUIRE(reinterpret_cast<uintptr_t>(state_out) % 16 == 0, "%s: state_out must be 16-byte aligned", op);
  MSCNN_REQUIRE(reinterpret_cast<uintptr_t>(track_ids_dev) % 4 == 0, "%s: track_ids_dev must be 4-byte aligned", op);
  const mscnn_tracks_state_layout SL = mscnn_tracks_state_layout_of(N * K, max_tracks);
  const size_t bytes = SL.total;
  const uintptr_t si = reinterpret_cast<uintptr_t>(state_in), so = reinterpret_cast<uintptr_t>(state_out);
  MSCNN_REQUIRE(si == so || si + bytes <= so || so + bytes <= si, "%s: state_in and state_out overlap (%zu bytes each) without being equal", op,
                bytes);
  size_t fbytes = 0;
  if (kc) {
    const uintptr_t fi = reinterpret_cast<uintptr_t>(kc->filter_in), fo = reinterpret_cast<uintptr_t>(kc->filter_out);
    MSCNN_REQUIRE(fi % 16 == 0, "%s: filter_in must be 16-byte aligned", op);
    MSCNN_REQUIRE(fo % 16 == 0, "%s: filter_out must be 16-byte aligned", op);
    fbytes = (size_t)N * (size_t)K * (size_t)max_tracks * sizeof(mscnn_track_kalman_record);
    MSCNN_REQUIRE(fi == fo || fi + fbytes <= fo || fo + fbytes <= fi, "%s: filter_in and filter_out overlap (%zu bytes each) without being equal", op,
                  fbytes);
    const uintptr_t fs[2] = {fi, fo}, ss[2] = {si, so};
    for (int i = 0; i < 2; ++i)
      for (int j = 0; j < 2; ++j)
        MSCNN_REQUIRE(fs[i] + fbytes <= ss[j] || ss[j] + bytes <= fs[i], "%s: %s (%zu bytes) overlaps %s (%zu bytes)", op,
                      i ? "filter_out" : "filter_in", fbytes, j ? "state_out" : "state_in", bytes);
  }
  TrackKalmanArgs ka = {};
  TrackArgs& a = ka;
  a.p = *p; a.num_frames = T; a.num_slots = K; a.cap = cap; a.max_tracks = max_tracks;
  a.pack = static_cast<const char*>(pack_dev); a.state_in = static_cast<const char*>(state_in); a.state_out = static_cast<char*>(state_out);
  a.ids = track_ids_dev;
  a.dets_at = mscnn_multi_pack_layout_of(T * K, cap).dets; a.slot_bytes = SL.slot; a.records_at = SL.records;
  a.num_streams = N;
  if (N > 1)
    for (int t = 0; t < T; ++t) a.stream_of[t] = (unsigned short)stream_of[t];      // (read here, before the call returns; T <= kTrackStreams)
  // the grid's y and z are bounded by 65535, x is not: the slots go to x
  if (kc) {
    const mscnn_track_kalman_params& f = *kc->filter;
    ka.sp = f.std_position; ka.sv = f.std_velocity; ka.sp2 = 2 * f.std_position; ka.sv10 = 10 * f.std_velocity;
    ka.a2 = f.std_aspect * f.std_aspect; ka.b2 = f.std_aspect_velocity * f.std_aspect_velocity; ka.m2 = f.std_aspect_measure * f.std_aspect_measure;
    ka.freeze_lost_height = f.freeze_lost_height;
    ka.filter_in = static_cast<const mscnn_track_kalman_record*>(kc->filter_in);
    ka.filter_out = static_cast<mscnn_track_kalman_record*>(kc->filter_out);
    if (assign == MSCNN_TRACK_ASSIGN_OPTIMAL)
      det_track_kernel<true, true, TrackKalmanArgs><<<dim3((unsigned)K, (unsigned)N), kTrackThreads, 0, as_stream(stream)>>>(ka);
    else
      det_track_kernel<true, false, TrackKalmanArgs><<<dim3((unsigned)K, (unsigned)N), kTrackThreads, 0, as_stream(stream)>>>(ka);
  } else {
    if (assign == MSCNN_TRACK_ASSIGN_OPTIMAL)
      det_track_kernel<false, true, TrackArgs><<<dim3((unsigned)K, (unsigned)N), kTrackThreads, 0, as_stream(stream)>>>(a);
    else
      det_track_kernel<false, false, TrackArgs><<<dim3((unsigned)K, (unsigned)N), kTrackThreads, 0, as_stream(stream)>>>(a);
  }
  MSCNN_POST_LAUNCH();
  return MSCNN_OK;
}

extern "C" int mscnn_tracks_update_fwd(const mscnn_track_params* p, int num_frames, int num_slots, const void* pack_dev, int cap,
                                       const void* state_in, void* state_out, int max_tracks, int* track_ids_dev, void* stream) {
  return tracks_update_any("tracks_update", false, p, num_frames, num_slots, 1, nullptr, pack_dev, cap, state_in, state_out, max_tracks,
                           track_ids_dev, stream);
}

extern "C" int mscnn_tracks_update_streams_fwd(const mscnn_track_params* p, int num_frames, int num_slots, int num_streams, const int* stream_of,
                                               const void* pack_dev, int cap, const void* state_in, void* state_out, int max_tracks,
                                               int* track_ids_dev, void* stream) {
  return tracks_update_any("tracks_update_streams", true, p, num_frames, num_slots, num_streams, stream_of, pack_dev, cap, state_in, state_out,
                           max_tracks, track_ids_dev, stream);
}

extern "C" size_t mscnn_tracks_kalman_state_bytes(int num_slots, int max_tracks) {
  if (!track_shape_ok(num_slots, max_tracks)) return 0;
  return (size_t)num_slots * (size_t)max_tracks * sizeof(mscnn_track_kalman_record);
}

extern "C" int mscnn_tracks_update_kalman_fwd(const mscnn_tracks_kalman_call* c) {
  MSCNN_REQUIRE(c, "tracks_update_kalman: null call");
  MSCNN_REQUIRE(c->size == sizeof(mscnn_tracks_kalman_call), "tracks_update_kalman: size %zu is not sizeof(mscnn_tracks_kalman_call) = %zu", c->size,
                sizeof(mscnn_tracks_kalman_call));
  return tracks_update_any("tracks_update_kalman", true, c->track, c->num_frames, c->num_slots, c->num_streams, c->stream_of, c->pack_dev, c->cap,
                           c->state_in, c->state_out, c->max_tracks, c->track_ids_dev, c->stream, c);
}

extern "C" int mscnn_tracks_update_assign_fwd(const mscnn_tracks_assign_call* c) {
  MSCNN_REQUIRE(c, "tracks_update_assign: null call");
  MSCNN_REQUIRE(c->size == sizeof(mscnn_tracks_assign_call), "tracks_update_assign: size %zu is not sizeof(mscnn_tracks_assign_call) = %zu", c->size,
                sizeof(mscnn_tracks_assign_call));
  MSCNN_REQUIRE(c->assign == MSCNN_TRACK_ASSIGN_GREEDY || c->assign == MSCNN_TRACK_ASSIGN_OPTIMAL,
                "tracks_update_assign: assign %d is neither %d (greedy) nor %d (optimal)", c->assign, MSCNN_TRACK_ASSIGN_GREEDY, MSCNN_TRACK_ASSIGN_OPTIMAL);
  if (!c->filter) {
    MSCNN_REQUIRE(!c->filter_in && !c->filter_out, "tracks_update_assign: %s is given without a filter", c->filter_in ? "filter_in" : "filter_out");
    return tracks_update_any("tracks_update_assign", true, c->track, c->num_frames, c->num_slots, c->num_streams, c->stream_of, c->pack_dev, c->cap,
                             c->state_in, c->state_out, c->max_tracks, c->track_ids_dev, c->stream, nullptr, c->assign, true);
  }
  mscnn_tracks_kalman_call kc = {};
  kc.size = sizeof(kc); kc.track = c->track; kc.filter = c->filter;
  kc.num_frames = c->num_frames; kc.num_slots = c->num_slots; kc.num_streams = c->num_streams; kc.stream_of = c->stream_of;
  kc.pack_dev = c->pack_dev; kc.cap = c->cap; kc.state_in = c->state_in; kc.state_out = c->state_out;
  kc.filter_in = c->filter_in; kc.filter_out = c->filter_out; kc.max_tracks = c->max_tracks; kc.track_ids_dev = c->track_ids_dev; kc.stream = c->stream;
  return tracks_update_any("tracks_update_assign", true, c->track, c->num_frames, c->num_slots, c->num_streams, c->stream_of, c->pack_dev, c->cap,
                           c->state_in, c->state_out, c->max_tracks, c->track_ids_dev, c->stream, &kc, c->assign);
}
