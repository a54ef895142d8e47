// Device arithmetic shared by the F(3x3,3x3) input transforms (winograd.hip, roipool_wino.hip): B^T d for one column / row of a
// 5 x 5 patch, interpolation points {0, 1, -1, 2, inf}.  One definition, so that every kernel that forms V = B^T d B rounds
// exactly alike (-ffp-contract=off: the expressions below are the operation order).
#pragma once
#include <hip/hip_runtime.h>

namespace mscnn {

__device__ __forceinline__ void bt5(const float d[5], float r[5]) {
  r[0] = 2.f * d[0] - d[1] - 2.f * d[2] + d[3];
  r[1] = -2.f * d[1] - d[2] + d[3];
  r[2] = 2.f * d[1] - 3.f * d[2] + d[3];
  r[3] = d[3] - d[1];
  r[4] = 2.f * d[1] - d[2] - 2.f * d[3] + d[4];
}

// Ragged planes of a small-map F(3x3,3x3) layer.  Plane index 4 (the point at infinity) feeds only the third output of a tile:
//   o0 = m0 + m1 + m2 + m3,  o1 = m1 - m2 + 2 m3,  o2 = m1 + m2 + 4 m3 + m4,
// so plane (i, j) with i == 4 is never read by a tile whose third output ROW lies outside the map (the last tile row when
// Ho % 3 != 0), and j == 4 likewise for the last tile column.  `ragged` is the grid description every kernel that touches such
// planes takes: bit 0 -- the planes (4, .) have one tile row less, bit 1 -- the planes (., 4) one tile column less; 0 -- every plane
// has the tiles_h x tiles_w grid.  Inside plane (i, j) the column of (image n, tile ty, tx) is (n th + ty) tw + tx over the plane's
// OWN grid (th, tw): the live columns of a plane are its first N th tw.
constexpr int kWino33RaggedRows = 1, kWino33RaggedCols = 2;
__host__ __device__ __forceinline__ int wino33_ragged_mode(int Ho, int Wo) {
  return (Ho % 3 != 0 ? kWino33RaggedRows : 0) | (Wo % 3 != 0 ? kWino33RaggedCols : 0);
}
__host__ __device__ __forceinline__ int wino33_plane_th(int ragged, int i, int tiles_h) {
  return tiles_h - ((i == 4 && (ragged & kWino33RaggedRows)) ? 1 : 0);
}
__host__ __device__ __forceinline__ int wino33_plane_tw(int ragged, int j, int tiles_w) {
  return tiles_w - ((j == 4 && (ragged & kWino33RaggedCols)) ? 1 : 0);
}

}  // namespace mscnn
