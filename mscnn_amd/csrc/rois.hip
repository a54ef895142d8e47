// Caller-supplied ROIs for gfx950: R rows become the two blobs BoxOutput would have written (box_output_layer.cpp:107,156:
// rois [image x1 y1 x2 y2], proposals_score [image x1 y1 x2 y2 score], rows grouped by image in ascending order), checked on the
// device because the rows may live there.  The formulas of the two input forms are in include/mscnn_hip.h (mscnn_rois_ingest_f32).
#include <climits>
#include <cmath>
#include <cstdint>
#include <type_traits>
#include "common.h"

namespace {

constexpr int kRoisThreads = 256;                                   // 4 waves: 256 rows per step
constexpr int kRoisWaves = kRoisThreads / 64;
constexpr int kRoisMaxImages = MSCNN_ROIS_MAX_RATIO_IMAGES;         // the ratios travel as kernel arguments (2 KB of the 4 KB)
struct RoisArgs {
  const void* rows; int R, num_images;
  float* rois; float* props;                                        // props may be null
  int* image_rows; int* status;
  double ratio_h[kRoisMaxImages], ratio_w[kRoisMaxImages];          // IMAGE form only
};
static_assert(sizeof(RoisArgs) <= 4096, "RoisArgs travels as kernel arguments");

__device__ __forceinline__ bool finite_f32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool finite_f64(double v) {
  return ((unsigned long long)__double_as_longlong(v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// first row of image >= img in rows that are known to be grouped by image (every row has passed the order check)
template <typename T>
__device__ __forceinline__ int rois_lower_bound(const T* __restrict__ rows, int R, int img) {
  int lo = 0, hi = R;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (rows[(size_t)mid * 6] < (T)img) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// One workgroup.  Steps of 256 rows: every lane judges its row, every wave ballots, the four first-bad rows meet in LDS.  A step with
// a bad row writes the verdict and ends the kernel: the rows of the steps before it have been written, no row of that step and
// none behind it.  The outputs are plain per-lane stores; the verdict is four of them by one lane (status may be host-coherent
// pinned memory: nothing here is read back, nothing is an atomic).
template <bool kImage>
__global__ __launch_bounds__(kRoisThreads) void rois_ingest_kernel(RoisArgs a) {
  using T = typename std::conditional<kImage, double, float>::type;
  __shared__ int s_bad[kRoisWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const T* __restrict__ in = static_cast<const T*>(a.rows);
  const int R = a.R, N = a.num_images;
  for (int c0 = 0; c0 < R; c0 += kRoisThreads) {
    const int r = c0 + tid;
    int reason = 0;
    float o[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (r < R) {
      const T* q = in + 6 * (size_t)r;
      T v[6];
      if constexpr (kImage) {
        for (int k = 0; k < 6; ++k) v[k] = q[k];
      } else {
        // a row is 24 bytes at a multiple of 24: three 8-byte loads, adjacent lanes adjacent rows
        const float2* q2 = reinterpret_cast<const float2*>(q);
        const float2 q0 = q2[0], q1 = q2[1], q3 = q2[2];
        v[0] = q0.x; v[1] = q0.y; v[2] = q1.x; v[3] = q1.y; v[4] = q3.x; v[5] = q3.y;
      }
      bool fin = true;
      for (int k = 0; k < 6; ++k) {
        if constexpr (kImage) fin = fin && finite_f64(v[k]); else fin = fin && finite_f32(v[k]);
      }
      const T img = v[0];
      const bool img_ok = fin && img >= (T)0 && img < (T)N && img == (T)(int)img;
      if (fin && img_ok) {
        if constexpr (kImage) {
          const int i = (int)img;
          const double rw = a.ratio_w[i], rh = a.ratio_h[i];
          o[0] = (float)img;
          o[1] = (float)(v[1] * rw);
          o[2] = (float)(v[2] * rh);
          o[3] = (float)((v[1] + v[3]) * rw);
          o[4] = (float)((v[2] + v[4]) * rh);
          o[5] = (float)v[5];
          for (int k = 1; k < 6; ++k) fin = fin && finite_f32(o[k]);      // (a product or a score past fp32's range)
        } else {
          for (int k = 0; k < 6; ++k) o[k] = v[k];                         // bit for bit
        }
      }
      if (!fin) reason = MSCNN_ROIS_BAD_NONFINITE;
      else if (!img_ok) reason = MSCNN_ROIS_BAD_IMAGE;
      else if (r > 0 && in[6 * (size_t)(r - 1)] > img) reason = MSCNN_ROIS_BAD_ORDER;      // (a NaN in front: that row's own verdict)
    }
    const unsigned long long m = __ballot(reason != 0);
    if (lane == 0) s_bad[wave] = m ? c0 + wave * 64 + (__ffsll((long long)m) - 1) : INT_MAX;
    __syncthreads();
    int first = INT_MAX;
    for (int w = 0; w < kRoisWaves; ++w) first = s_bad[w] < first ? s_bad[w] : first;
    if (first != INT_MAX) {
      if (r == first) { a.status[0] = 0; a.status[1] = r; a.status[2] = reason; a.status[3] = 0; }
      return;      // (uniform: every thread has read the same four words)
    }
    if (r < R) {
      float* d = a.rois + 5 * (size_t)r;
      for (int k = 0; k < 5; ++k) d[k] = o[k];
      if (a.props) {
        float* p = a.props + 6 * (size_t)r;
        for (int k = 0; k < 6; ++k) p[k] = o[k];
      }
    }
    __syncthreads();      // every thread has read s_bad before the next step writes it
  }
  // every row is good: the rows are grouped, so an image's count is the distance of two lower bounds in the input
  for (int i = tid; i < N; i += kRoisThreads) a.image_rows[i] = rois_lower_bound(in, R, i + 1) - rois_lower_bound(in, R, i);
  if (tid == 0) { a.status[0] = 1; a.status[1] = -1; a.status[2] = 0; a.status[3] = 0; }
}
}  // namespace

using namespace mscnn;

extern "C" const char* mscnn_rois_reason_text(int reason) {
  switch (reason) {
    case MSCNN_ROIS_BAD_NONFINITE: return "a value that is not finite";
    case MSCNN_ROIS_BAD_IMAGE: return "an image index outside [0, num_images) or not a whole number";
    case MSCNN_ROIS_BAD_ORDER: return "an image index smaller than the row's in front of it (rows must be grouped by image)";
    default: return "no error";
  }
}

extern "C" int mscnn_rois_ingest_f32(const void* rows, int coords, int R, int num_images, const double* ratio_h, const double* ratio_w,
                                     float* rois, float* props, int* image_rows, int* status, void* stream) {
  MSCNN_REQUIRE(rows != nullptr, "rois_ingest: null pointer: rows");
  MSCNN_REQUIRE(rois != nullptr, "rois_ingest: null pointer: rois");
  MSCNN_REQUIRE(image_rows != nullptr, "rois_ingest: null pointer: image_rows");
  MSCNN_REQUIRE(status != nullptr, "rois_ingest: null pointer: status");
  MSCNN_REQUIRE(coords == MSCNN_ROIS_NET || coords == MSCNN_ROIS_IMAGE, "rois_ingest: coords = %d (MSCNN_ROIS_NET 0 or MSCNN_ROIS_IMAGE 1)",
                coords);
  MSCNN_REQUIRE(R >= 1, "rois_ingest: R = %d (at least one row)", R);
  MSCNN_REQUIRE(num_images >= 1 && num_images <= (1 << 24), "rois_ingest: N = %d images (1 .. %d)", num_images, 1 << 24);
  MSCNN_REQUIRE_ALIGNED(rows, 8, "rois_ingest: rows");
  MSCNN_REQUIRE_ALIGNED(rois, 4, "rois_ingest: rois");
  MSCNN_REQUIRE_ALIGNED(props, 4, "rois_ingest: props");
  MSCNN_REQUIRE_ALIGNED(image_rows, 4, "rois_ingest: image_rows");
  MSCNN_REQUIRE_ALIGNED(status, 4, "rois_ingest: status");
  RoisArgs a = {};
  a.rows = rows; a.R = R; a.num_images = num_images;
  a.rois = rois; a.props = props; a.image_rows = image_rows; a.status = status;
  hipStream_t st = as_stream(stream);
  if (coords == MSCNN_ROIS_IMAGE) {
    MSCNN_REQUIRE(ratio_h != nullptr && ratio_w != nullptr, "rois_ingest: null pointer: ratio_h / ratio_w (MSCNN_ROIS_IMAGE)");
    MSCNN_REQUIRE(num_images <= kRoisMaxImages, "rois_ingest: N = %d images with MSCNN_ROIS_IMAGE (at most %d: the ratios travel with the launch)",
                  num_images, kRoisMaxImages);
    for (int i = 0; i < num_images; ++i) {
      MSCNN_REQUIRE(ratio_h[i] > 0 && ratio_w[i] > 0 && std::isfinite(ratio_h[i]) && std::isfinite(ratio_w[i]),
                    "rois_ingest: image %d: ratios %g x %g (positive finite numbers)", i, ratio_h[i], ratio_w[i]);
      a.ratio_h[i] = ratio_h[i]; a.ratio_w[i] = ratio_w[i];
    }
    rois_ingest_kernel<true><<<1, kRoisThreads, 0, st>>>(a);
  } else {
    rois_ingest_kernel<false><<<1, kRoisThreads, 0, st>>>(a);
  }
  MSCNN_POST_LAUNCH();
  return MSCNN_OK;
}
