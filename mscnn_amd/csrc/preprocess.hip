// Image pre-processing in front of net.forward, on the device.
// Replaces the MATLAB lines examples/kitti_car/run_mscnn_detection.m:64-69:
//     test_image = imresize(test_image,[imgH imgW]); test_image = single(test_image(:,:,[3 2 1]));
//     test_image = bsxfun(@minus,test_image,mu);    test_image = permute(test_image, [2 1 3]);
// imresize is restated from its published algorithm (bicubic a = -0.5, kernel stretched by 1/scale when shrinking,
// P = ceil(width) + 2 taps, normalised weights, symmetric border mirroring, smaller-scale dimension first, uint8 rounding
// after EACH 1-D pass) -- MATLAB itself is not available, so this stage is "parity unpinned" like the final detection stage;
// it is bit-identical to oracle/pyoracle.py::preprocess (same double-precision operation order; -ffp-contract=off).
// Two HBM-bound kernels: pass 1 resizes along the first dimension into a uint8 scratch image, pass 2 resizes along the
// other one and fuses the RGB->BGR swap, the mean subtraction and the HWC -> NCHW layout change.  Both take a batch: a table of
// up to kMaxImages frames of their own sizes (and so their own pass order and intermediate) passed by value as a kernel argument,
// blockIdx.y = the frame's slot.  The single-frame op is a batch of one.
#include "common.h"
#include <cstdint>
#include <vector>

namespace {

__device__ __forceinline__ double cubic(double x) {
  const double ax = fabs(x), ax2 = ax * ax, ax3 = ax2 * ax;
  if (ax <= 1.0) return (1.5 * ax3 - 2.5 * ax2) + 1.0;
  if (ax <= 2.0) return ((-0.5 * ax3 + 2.5 * ax2) - 4.0 * ax) + 2.0;
  return 0.0;
}

// 1-D resize of output index `o` (0-based): calls f(k, weight, source index) for the P taps in order
struct Taps {
  double scale, kw, u, left, sum;
  int P, in_len;
  __device__ Taps(int in_len_, int out_len, int o) : in_len(in_len_) {
    scale = (double)out_len / (double)in_len_;
    kw = scale < 1.0 ? 4.0 / scale : 4.0;
    const double x = (double)(o + 1);
    u = x / scale + 0.5 * (1.0 - 1.0 / scale);
    left = floor(u - kw / 2.0);
    P = (int)ceil(kw) + 2;
    sum = 0.0;
    for (int k = 0; k < P; ++k) sum = sum + raw(k);
  }
  __device__ double raw(int k) const {
    const double d = u - (left + (double)k);
    return scale < 1.0 ? scale * cubic(scale * d) : cubic(d);
  }
  __device__ int index(int k) const {            // symmetric mirroring: aux = [1..n, n..1]
    const long period = 2L * in_len;
    long m = ((long)left + k - 1) % period;
    if (m < 0) m += period;
    return (int)(m < in_len ? m : period - 1 - m);
  }
};

__device__ __forceinline__ unsigned char to_u8(double v) {
  v = floor(v + 0.5);
  return (unsigned char)(v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v));
}

// One image of a launch.  Pass 1 resizes src [org_h][org_w][3] into mid [mh][mw][3] along H (h_first) or along W; pass 2 resizes
// mid along the other axis into the image's [3][H][W] slice of the output.
struct PreImage {
  const unsigned char* src;
  unsigned char* mid;
  int org_h, org_w, mh, mw, h_first;
};
constexpr int kMaxImages = 32;              // images per launch: the table is 32 x 40 B = 1280 B of kernel arguments
struct PreTable { PreImage img[kMaxImages]; };

// src [sh][sw][3] u8 -> dst [dh][sw][3] u8 (resize along H) or [sh][dw][3] (along W); element i of dst
template <int ALONG_W>
__device__ __forceinline__ void resize_u8_elem(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int sh, int sw,
                                               int dh, int dw, long i) {
  const int c = (int)(i % 3), x = (int)((i / 3) % dw), y = (int)(i / (3L * dw));
  Taps t(ALONG_W ? sw : sh, ALONG_W ? dw : dh, ALONG_W ? x : y);
  double acc = 0.0;
  for (int k = 0; k < t.P; ++k) {
    const int s = t.index(k);
    const double v = ALONG_W ? (double)src[((long)y * sw + s) * 3 + c] : (double)src[((long)s * sw + x) * 3 + c];
    acc = acc + (t.raw(k) / t.sum) * v;
  }
  dst[i] = to_u8(acc);
}

// last pass fused with BGR swap + mean subtraction + layout: src [sh][sw][3] u8 RGB -> out [3][dh][dw] f32 (BGR planes); pixel i
template <int ALONG_W>
__device__ __forceinline__ void resize_finish_elem(const unsigned char* __restrict__ src, float* __restrict__ out, int sh, int sw,
                                                   int dh, int dw, float mb, float mg, float mr, long i) {
  const long total = (long)dh * dw;
  const int x = (int)(i % dw), y = (int)(i / dw);
  Taps t(ALONG_W ? sw : sh, ALONG_W ? dw : dh, ALONG_W ? x : y);
  double acc[3] = {0.0, 0.0, 0.0};
  for (int k = 0; k < t.P; ++k) {
    const int s = t.index(k);
    const unsigned char* p = ALONG_W ? src + ((long)y * sw + s) * 3 : src + ((long)s * sw + x) * 3;
    const double w = t.raw(k) / t.sum;
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = acc[c] + w * (double)p[c];
  }
  out[i] = (float)to_u8(acc[2]) - mb;                 // plane 0 = B
  out[total + i] = (float)to_u8(acc[1]) - mg;         // plane 1 = G
  out[2 * total + i] = (float)to_u8(acc[0]) - mr;     // plane 2 = R
}

// pass 1 of every image of the table: blockIdx.y = image slot, grid-stride over that image's intermediate along x
__global__ __launch_bounds__(256) void resize_u8_batch_kernel(const PreTable tab) {
  const PreImage& d = tab.img[blockIdx.y];
  const long total = (long)d.mh * d.mw * 3;
  const long step = (long)gridDim.x * 256;
  if (d.h_first) {                                    // uniform per block
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += step) resize_u8_elem<0>(d.src, d.mid, d.org_h, d.org_w, d.mh, d.mw, i);
  } else {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += step) resize_u8_elem<1>(d.src, d.mid, d.org_h, d.org_w, d.mh, d.mw, i);
  }
}

// pass 2 of every image of the table: slot s writes out + s * 3 * H * W
__global__ __launch_bounds__(256) void resize_finish_batch_kernel(const PreTable tab, float* __restrict__ out, int H, int W, float mb,
                                                                  float mg, float mr) {
  const PreImage& d = tab.img[blockIdx.y];
  const long total = (long)H * W;
  const long step = (long)gridDim.x * 256;
  float* o = out + (long)blockIdx.y * 3 * total;
  if (d.h_first) {                                    // H done in pass 1: along W here
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += step) resize_finish_elem<1>(d.mid, o, d.mh, d.mw, H, W, mb, mg, mr, i);
  } else {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += step) resize_finish_elem<0>(d.mid, o, d.mh, d.mw, H, W, mb, mg, mr, i);
  }
}

// [~, order] = sort(scale): the smaller scale first
inline bool h_first_of(int org_h, int org_w, int H, int W) { return (double)H / org_h <= (double)W / org_w; }

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// imgs[0..n) with their intermediates mid[0..n) -> out [n][3][H][W]: two launches per chunk of kMaxImages images
int preprocess_launch(const unsigned char* const* imgs, unsigned char* const* mids, const int* org_h, const int* org_w, int n, float* out,
                      int H, int W, const float* mean_bgr, hipStream_t st) {
  for (int c0 = 0; c0 < n; c0 += kMaxImages) {
    const int m = n - c0 < kMaxImages ? n - c0 : kMaxImages;
    PreTable tab = {};
    long mid_max = 0;
    for (int s = 0; s < m; ++s) {
      const int b = c0 + s;
      const bool hf = h_first_of(org_h[b], org_w[b], H, W);
      tab.img[s] = PreImage{imgs[b], mids[b], org_h[b], org_w[b], hf ? H : org_h[b], hf ? org_w[b] : W, hf ? 1 : 0};
      const long e = (long)tab.img[s].mh * tab.img[s].mw * 3;
      if (e > mid_max) mid_max = e;
    }
    long blocks = (mid_max + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    resize_u8_batch_kernel<<<dim3((unsigned)blocks, (unsigned)m), 256, 0, st>>>(tab);
    MSCNN_POST_LAUNCH();
    blocks = ((long)H * W + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    resize_finish_batch_kernel<<<dim3((unsigned)blocks, (unsigned)m), 256, 0, st>>>(tab, out + (long)c0 * 3 * H * W, H, W, mean_bgr[0],
                                                                                   mean_bgr[1], mean_bgr[2]);
    MSCNN_POST_LAUNCH();
  }
  return MSCNN_OK;
}

// ---- views: windows of uploaded frames, optionally mirrored, as the images of one batch (mscnn_preprocess_views_u8_f32) -------------
// A view's first pass reads its window where it lies: win = the window's first pixel in its frame, pitch = the frame's row in
// pixels, and the mirrored column is part of the tap's source index.  The taps are those of a w x h image (Taps mirrors at the
// window's own borders, so no pixel outside the window is read), the intermediate is the window's own, and the second pass is
// resize_finish_batch_kernel above on that intermediate: it never sees the frame.
struct PreView {
  const unsigned char* win;
  unsigned char* mid;
  int pitch, w, h, mh, mw, h_first, flip_x;
};
struct PreViewTable { PreView view[kMaxImages]; };      // 32 x 48 B = 1536 B of kernel arguments

// window [h][w] of a frame -> mid [mh][w][3] (resize along H) or [h][mw][3] (along W); element i of mid
template <int ALONG_W>
__device__ __forceinline__ void resize_u8_view_elem(const PreView& d, long i) {
  const int c = (int)(i % 3), x = (int)((i / 3) % d.mw), y = (int)(i / (3L * d.mw));
  Taps t(ALONG_W ? d.w : d.h, ALONG_W ? d.mw : d.mh, ALONG_W ? x : y);
  double acc = 0.0;
  for (int k = 0; k < t.P; ++k) {
    const int s = t.index(k);
    const int row = ALONG_W ? y : s, col = ALONG_W ? s : x;
    const double v = (double)d.win[((long)row * d.pitch + (d.flip_x ? d.w - 1 - col : col)) * 3 + c];
    acc = acc + (t.raw(k) / t.sum) * v;
  }
  d.mid[i] = to_u8(acc);
}

// pass 1 of every view of the table: blockIdx.y = the view's slot, grid-stride over that view's intermediate along x
__global__ __launch_bounds__(256) void resize_u8_views_kernel(const PreViewTable tab) {
  const PreView& d = tab.view[blockIdx.y];
  const long total = (long)d.mh * d.mw * 3;
  const long step = (long)gridDim.x * 256;
  if (d.h_first) {                                    // uniform per block
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += step) resize_u8_view_elem<0>(d, i);
  } else {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += step) resize_u8_view_elem<1>(d, i);
  }
}

size_t view_mid_bytes(const mscnn_preprocess_view& v, int H, int W) {
  return h_first_of(v.h, v.w, H, W) ? (size_t)H * v.w * 3 : (size_t)v.h * W * 3;
}

}  // namespace

using namespace mscnn;

extern "C" size_t mscnn_preprocess_workspace_bytes(int org_h, int org_w, int H, int W) {
  // the intermediate image after the first 1-D pass
  return h_first_of(org_h, org_w, H, W) ? (size_t)H * org_w * 3 : (size_t)org_h * W * 3;
}

extern "C" int mscnn_preprocess_u8_f32(const unsigned char* img_rgb, int org_h, int org_w, float* out, int H, int W,
                                       const float* mean_bgr, void* workspace, size_t workspace_bytes, void* stream) {
  MSCNN_REQUIRE(img_rgb && out && mean_bgr, "preprocess: null pointer");
  MSCNN_REQUIRE(org_h > 0 && org_w > 0 && H > 0 && W > 0, "preprocess: bad shape");
  MSCNN_REQUIRE(workspace && workspace_bytes >= mscnn_preprocess_workspace_bytes(org_h, org_w, H, W), "preprocess: workspace too small");
  MSCNN_REQUIRE_ALIGNED(workspace, 16, "preprocess: workspace");
  unsigned char* mid = static_cast<unsigned char*>(workspace);
  return preprocess_launch(&img_rgb, &mid, &org_h, &org_w, 1, out, H, W, mean_bgr, as_stream(stream));
}

extern "C" size_t mscnn_preprocess_batch_workspace_bytes(int count, const int* org_h, const int* org_w, int H, int W) {
  // every image's intermediate at a 256-byte aligned offset, back to back; 0 for arguments the op refuses
  if (count < 1 || !org_h || !org_w || H <= 0 || W <= 0) return 0;
  size_t total = 0;
  for (int b = 0; b < count; ++b) {
    if (org_h[b] <= 0 || org_w[b] <= 0) return 0;
    total += align256(mscnn_preprocess_workspace_bytes(org_h[b], org_w[b], H, W));
  }
  return total;
}

extern "C" int mscnn_preprocess_batch_u8_f32(const unsigned char* const* imgs_rgb, const int* org_h, const int* org_w, int count,
                                             float* out, int H, int W, const float* mean_bgr, void* workspace, size_t workspace_bytes,
                                             void* stream) {
  MSCNN_REQUIRE(imgs_rgb && org_h && org_w && out && mean_bgr && workspace, "preprocess_batch: null pointer");
  MSCNN_REQUIRE(count >= 1, "preprocess_batch: count %d < 1", count);
  MSCNN_REQUIRE_ALIGNED(workspace, 16, "preprocess_batch: workspace");
  MSCNN_REQUIRE(H > 0 && W > 0, "preprocess_batch: bad output shape %d x %d", H, W);
  for (int b = 0; b < count; ++b) {
    MSCNN_REQUIRE(org_h[b] > 0 && org_w[b] > 0, "preprocess_batch: image %d has bad shape %d x %d", b, org_h[b], org_w[b]);
    MSCNN_REQUIRE(imgs_rgb[b], "preprocess_batch: image %d is a null pointer", b);
  }
  const size_t need = mscnn_preprocess_batch_workspace_bytes(count, org_h, org_w, H, W);
  MSCNN_REQUIRE(workspace_bytes >= need, "preprocess_batch: workspace %zu bytes < %zu", workspace_bytes, need);
  std::vector<unsigned char*> mids(count);
  size_t off = 0;
  for (int b = 0; b < count; ++b) {
    mids[b] = static_cast<unsigned char*>(workspace) + off;
    off += align256(mscnn_preprocess_workspace_bytes(org_h[b], org_w[b], H, W));
  }
  return preprocess_launch(imgs_rgb, mids.data(), org_h, org_w, count, out, H, W, mean_bgr, as_stream(stream));
}

extern "C" size_t mscnn_preprocess_views_workspace_bytes(const mscnn_preprocess_view* views, int count, int H, int W) {
  // every view's intermediate at a 256-byte aligned offset, back to back; 0 for arguments the op refuses
  if (count < 1 || !views || H <= 0 || W <= 0) return 0;
  size_t total = 0;
  for (int v = 0; v < count; ++v) {
    if (views[v].w < 1 || views[v].h < 1) return 0;
    total += align256(view_mid_bytes(views[v], H, W));
  }
  return total;
}

extern "C" int mscnn_preprocess_views_u8_f32(const unsigned char* const* frames_rgb, const int* org_h, const int* org_w, int num_frames,
                                             const mscnn_preprocess_view* views, int count, float* out, int H, int W,
                                             const float* mean_bgr, void* workspace, size_t workspace_bytes, void* stream) {
  MSCNN_REQUIRE(frames_rgb && org_h && org_w && views && out && mean_bgr && workspace, "preprocess_views: null pointer");
  MSCNN_REQUIRE(count >= 1, "preprocess_views: count %d < 1", count);
  MSCNN_REQUIRE(num_frames >= 1, "preprocess_views: num_frames %d < 1", num_frames);
  MSCNN_REQUIRE_ALIGNED(workspace, 16, "preprocess_views: workspace");
  MSCNN_REQUIRE(H > 0 && W > 0, "preprocess_views: bad output shape %d x %d", H, W);
  for (int f = 0; f < num_frames; ++f) {
    MSCNN_REQUIRE(org_h[f] > 0 && org_w[f] > 0, "preprocess_views: frame %d has bad shape %d x %d", f, org_h[f], org_w[f]);
    MSCNN_REQUIRE(frames_rgb[f], "preprocess_views: frame %d is a null pointer", f);
  }
  for (int v = 0; v < count; ++v) {
    const mscnn_preprocess_view& q = views[v];
    MSCNN_REQUIRE(q.frame >= 0 && q.frame < num_frames, "preprocess_views: view %d: frame %d outside [0, %d)", v, q.frame, num_frames);
    MSCNN_REQUIRE(q.w >= 1 && q.h >= 1, "preprocess_views: view %d: window %d x %d (h x w) is empty", v, q.h, q.w);
    MSCNN_REQUIRE(q.x0 >= 0 && q.y0 >= 0 && (long)q.x0 + q.w <= (long)org_w[q.frame] && (long)q.y0 + q.h <= (long)org_h[q.frame],
                  "preprocess_views: view %d: window %d x %d (h x w) at (x0 %d, y0 %d) is not inside frame %d of %d x %d", v, q.h, q.w, q.x0,
                  q.y0, q.frame, org_h[q.frame], org_w[q.frame]);
    MSCNN_REQUIRE(q.flip_x == 0 || q.flip_x == 1, "preprocess_views: view %d: flip_x %d (0 or 1)", v, q.flip_x);
  }
  const size_t need = mscnn_preprocess_views_workspace_bytes(views, count, H, W);
  MSCNN_REQUIRE(workspace_bytes >= need, "preprocess_views: workspace %zu bytes < %zu", workspace_bytes, need);
  hipStream_t st = as_stream(stream);
  size_t off = 0;
  for (int c0 = 0; c0 < count; c0 += kMaxImages) {
    const int m = count - c0 < kMaxImages ? count - c0 : kMaxImages;
    PreViewTable vt = {};
    PreTable tab = {};
    long mid_max = 0;
    for (int s = 0; s < m; ++s) {
      const mscnn_preprocess_view& q = views[c0 + s];
      const bool hf = h_first_of(q.h, q.w, H, W);
      const int pitch = org_w[q.frame];
      unsigned char* mid = static_cast<unsigned char*>(workspace) + off;
      off += align256(view_mid_bytes(q, H, W));
      vt.view[s] = PreView{frames_rgb[q.frame] + ((long)q.y0 * pitch + q.x0) * 3, mid, pitch, q.w, q.h, hf ? H : q.h, hf ? q.w : W, hf ? 1 : 0,
                           q.flip_x};
      tab.img[s] = PreImage{nullptr, mid, q.h, q.w, vt.view[s].mh, vt.view[s].mw, hf ? 1 : 0};      // (the second pass reads mid only)
      const long e = (long)vt.view[s].mh * vt.view[s].mw * 3;
      if (e > mid_max) mid_max = e;
    }
    long blocks = (mid_max + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    resize_u8_views_kernel<<<dim3((unsigned)blocks, (unsigned)m), 256, 0, st>>>(vt);
    MSCNN_POST_LAUNCH();
    blocks = ((long)H * W + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    resize_finish_batch_kernel<<<dim3((unsigned)blocks, (unsigned)m), 256, 0, st>>>(tab, out + (long)c0 * 3 * H * W, H, W, mean_bgr[0],
                                                                                   mean_bgr[1], mean_bgr[2]);
    MSCNN_POST_LAUNCH();
  }
  return MSCNN_OK;
}
