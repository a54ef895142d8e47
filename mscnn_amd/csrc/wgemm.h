// Internal interface of wgemm.hip: the batched transform-domain GEMM of the Winograd convolution paths,
//   M[p][Cout][T_pad] = U[p][Cout][Cin] x V[p][Cin][T_pad]     for the P = (m+2)^2 transform planes of F(m x m, 3x3).
// It replaces the 1x1 igemm kernel that ran these GEMMs in rounds 1-2 (conv.hip) -- see the header of wgemm.hip for why.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

namespace mscnn {

constexpr int kWgemmMaxPlanes = 36;

// Tile index -> (plane, column tile, row tile): t = (nt_off[p] + nt) * MT + mt, with nt_off[p] = p * NT when every plane has the same
// NT column tiles (nt_off == nullptr).  The ONE decode of the kernel's producer and consumer and of the host-side checks.
__host__ __device__ __forceinline__ void wgemm_tile_decode(int t, int MT, int NT, int P, const int* nt_off, int& p, int& nt, int& mt) {
  mt = t % MT;
  if (!nt_off) {
    nt = (t / MT) % NT;
    p = t / (MT * NT);
    return;
  }
#if defined(__HIP_DEVICE_COMPILE__)
  const int q = __builtin_amdgcn_readfirstlane(t / MT);      // (t is wave-uniform: keeps the scan over the table on the scalar unit)
#else
  const int q = t / MT;
#endif
  int pp = 0;
  while (pp + 1 < P && nt_off[pp + 1] <= q) ++pp;
  p = pp;
  nt = q - nt_off[pp];
}

struct WgemmPlan {
  int P, Cout, Cin, T, T_pad;       // T_pad: row stride of V and M (multiple of the N tile)
  int BM, BN, CK, MT, NT, KI;       // tile shape, tiles per plane, K chunks
  int G;                            // persistent grid (workgroups)
  int tiles;                        // MT x (column tiles of all planes): P MT NT for uniform planes
  // ragged planes (wgemm_plan with per-plane column counts): plane p has cols[p] live columns at its front and its own number of
  // column tiles; nt_off[p] = column tiles of the planes before p (nt_off[P] = all of them).  ragged == 0: every plane has NT.
  int ragged;
  int cols[kWgemmMaxPlanes];
  int nt_off[kWgemmMaxPlanes + 1];
  int device;                       // the device G was taken from (-1: planned without one); wgemm_launch refuses another
  int full_q;                       // whole tiles per workgroup; the remaining tiles are split stream-K style
  int variant;
  double model_us;                  // the plan's own time estimate (picks between tile shapes)
  const char* name;
  size_t packed_bytes;              // U in the packed layout Up[p][mt][kc][ck][BM]
  size_t ws_bytes;                  // partial-tile slabs of the stream-K phase
};

// variant 0: pick per shape (bits 8 / 9 of variant: development -- force the stream-K split / whole tiles).  Returns false when no
// kernel covers the shape (the caller keeps the igemm path).
// plane_cols != nullptr: plane p has plane_cols[p] <= T live columns (at its front; P <= kWgemmMaxPlanes entries) and only
// ceil(plane_cols[p] / BN) column tiles; T_pad, the packing and the buffer limits still come from T.
bool wgemm_plan(int P, int Cout, int Cin, int T, int variant, WgemmPlan* out, const int* plane_cols = nullptr);

// abl: development ablations (0 in the product): bit 0 no loads after the prologue, bit 1 no stores, bit 2 no MFMAs, bit 3 no
// LDS operand reads, bit 4 no barriers; dbg: per-workgroup {shader cycles, 100 MHz ticks} (tools/micro/wgemm_bench.hip)
// bias / relu: only for a plan of an epilogue variant (variant + 64: InnerProduct on this kernel; bias indexed by column);
// m_valid_bytes != 0: the bytes of M that exist (Cout was rounded up to the tile grid's 32-row blocks, the caller's buffer was not)
int wgemm_launch(const WgemmPlan& p, const float* Up, const float* V, float* M, float* ws, hipStream_t st, int abl = 0,
                 unsigned long long* dbg = nullptr, const float* bias = nullptr, int relu = 0, size_t m_valid_bytes = 0);

// Hand-off health (mscnn_hip.h: mscnn_wgemm_handoff_event & co).  event: the epoch of the last launch on the current device whose
// finisher gave up on a contributor (0: none yet) -- read it after synchronising the stream.
unsigned long long wgemm_handoff_event();
void wgemm_force_whole_tiles(int on);
int wgemm_whole_tiles_forced();
void wgemm_debug_handoff_fault(int drop_publish, unsigned spin_limit);
// Host-side replay of the schedule (tests): every (tile, chunk) unit the G slots' segment cursors hand out, in slot order, as
// rows {slot, p, nt, mt, k0, k1, part} -- returns the number of segments (out may be nullptr to count), -1 when max_rows is too small.
long wgemm_debug_schedule(const WgemmPlan& p, int whole_tiles, int* out, long max_rows);

}  // namespace mscnn
