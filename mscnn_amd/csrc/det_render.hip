// The render stage (mscnn_render_detections_u8): the scripts' `show` block for the frames of a multi pack, in one device pass --
// outlines, fill, labels (score, track id) and the pixelation of box interiors.  include/mscnn_hip.h carries the contract; this
// file restates nothing of it but the segment's row-offset rule (render_segment, the rule of det_track.hip's step 2).
// Parallel over PIXELS, so that the paint order needs no atomics and no order between workgroups: a workgroup of kRenderThreads owns
// a kTileW x kTileH tile of one frame, a thread four of its pixels (one column, every fourth row) in registers.  The workgroup walks
// the frame's rows in paint order, kRenderThreads at a time: thread i forms row i's footprint and label, the rows that meet the tile
// are compacted IN ORDER into LDS (ballots and popcounts, as track_rank in det_track.hip), every pixel walks that short list, then
// the next chunk -- the order holds across chunks because a chunk is painted before the next is formed.
// Every loop bound and every value that guards a barrier is a kernel argument or a pack word clamped against cap, read alike by
// every thread of the workgroup.  Integer arithmetic from the rounding on; the doubles in front of it one statement per operation.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"
#include "render_glyphs.h"

namespace {
typedef unsigned long long u64;

constexpr int kRenderThreads = 256, kRenderWaves = kRenderThreads / 64;
constexpr int kTileW = 64, kTileH = 16, kPixPerThread = kTileH / kRenderWaves;      // a wave = one row of the tile
constexpr int kRenderFrames = MSCNN_RENDER_FRAMES_PER_LAUNCH;
// (a label holds at most 15 characters -- the 10 digits of an int32, a blank, "0.NN" --, 4 bits each in RenderItem's one 64-bit word)
constexpr double kMaxMagnitude = 1073741824.0;      // 2^30

__constant__ unsigned char d_glyph[MSCNN_RENDER_GLYPHS][7] = MSCNN_RENDER_GLYPH_ROWS;
const unsigned char h_glyph[MSCNN_RENDER_GLYPHS][7] = MSCNN_RENDER_GLYPH_ROWS;

struct RenderFrame { const unsigned char* src; unsigned char* dst; int h, w; };
struct RenderArgs {
  mscnn_render_params p;
  RenderFrame frame[kRenderFrames];      // 32 x 24 B by value
  int t0, num_slots, cap;                // t0: the pack's frame of frame[0]
  size_t dets_at;
  const char* pack;
  const int* ids;
};

// a drawn row that meets the tile: the box, the label rectangle (lw 0: none), the colour (bit 24: white ink) and the text
struct RenderItem { int L, T, R, B, ll, lt, lw; unsigned col; u64 txt; };

// the places of the set flags among the workgroup's threads, and their number (every thread calls it; two barriers)
__device__ __forceinline__ int render_rank(bool on, int* wsum, int* total_out) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u64 bits = __ballot(on);
  if (lane == 0) wsum[wave] = __popcll(bits);
  __syncthreads();
  int before = 0, total = 0;
  for (int c = 0; c < kRenderWaves; ++c) {
    const int v = wsum[c];
    before += c < wave ? v : 0;
    total += v;
  }
  __syncthreads();      // (wsum is free again)
  *total_out = total;
  return before + __popcll(bits & ((1ull << lane) - 1ull));
}

// Segment t * K + k of the pack: its row offset and its number of rows, 0 for a segment that counts as empty.  The rule of
// mscnn_tracks_update_fwd's step 2; on return 0 <= *off and *off + rows <= cap.
__device__ __forceinline__ int render_segment(const int* hdr, int K, int t, int k, int cap, long long* off_out) {
  const int* ent = hdr + MSCNN_MULTI_PACK_WORDS * ((size_t)1 + (size_t)t * K + k);
  const int count = ent[0];
  long long off = ent[2];
  if (K >= 2) {      // an image's slots share row0 (mscnn_detections_multi_fwd); a merged list has a row offset of its own
    const int* e0 = hdr + MSCNN_MULTI_PACK_WORDS * ((size_t)1 + (size_t)t * K);
    if (e0[2] == e0[MSCNN_MULTI_PACK_WORDS + 2]) off = (long long)K * ent[2] + (long long)k * ent[1];
  }
  const bool fits = count >= 0 && off >= 0 && off + (long long)count <= (long long)cap;
  *off_out = fits ? off : 0;
  return fits ? count : 0;
}

__device__ __forceinline__ int render_blend(int v, int c, int a) { return (v * (256 - a) + c * a + 128) >> 8; }

// One pack row as a RenderItem for a frame of h x w pixels.  false: not drawn.
__device__ __forceinline__ bool render_item(const mscnn_render_params& p, const double* d, int id, int k, int h, int w, RenderItem* out) {
  const double x = d[0], y = d[1], bw = d[2], bh = d[3], sc = d[4];
  if (!(sc >= p.show_thr)) return false;
  if (!(isfinite(x) && isfinite(y) && isfinite(bw) && isfinite(bh) && isfinite(sc))) return false;
  if (fabs(x) > kMaxMagnitude || fabs(y) > kMaxMagnitude || fabs(bw) > kMaxMagnitude || fabs(bh) > kMaxMagnitude) return false;
  const double xe = x + bw, ye = y + bh;
  const double fl = floor(x + 0.5), ft = floor(y + 0.5), fr = floor(xe + 0.5) - 1.0, fb = floor(ye + 0.5) - 1.0;
  if (fr < fl || fb < ft) return false;
  RenderItem it;
  it.L = (int)fl; it.T = (int)ft; it.R = (int)fr; it.B = (int)fb;      // (inside [-2^30, 2^31 - 1])
  if (it.L > w - 1 || it.R < 0 || it.T > h - 1 || it.B < 0) return false;      // the box holds no pixel of the frame
  const bool by_id = p.color_by == 1 && id > 0;
  const unsigned char* c = p.colors[(by_id ? id : k) % p.num_colors];
  const int lum = 299 * c[0] + 587 * c[1] + 114 * c[2];
  it.col = (unsigned)c[0] | ((unsigned)c[1] << 8) | ((unsigned)c[2] << 16) | (lum >= 128000 ? 0u : 1u << 24);
  int nch = 0;
  u64 txt = 0;
  if (p.label >= 2 && id > 0) {
    for (int v = id; v > 0; v /= 10) ++nch;
    int v = id;
    for (int q = nch - 1; q >= 0; --q) { txt |= (u64)(v % 10) << (4 * q); v /= 10; }
  }
  if (p.label == 1 || p.label == 3) {
    const double s100 = sc * 100.0;
    const double f = floor(s100 + 0.5);
    const int cc = f < 0.0 ? 0 : (f > 100.0 ? 100 : (int)f);
    if (nch) { txt |= (u64)MSCNN_RENDER_GLYPH_BLANK << (4 * nch); ++nch; }
    txt |= (u64)(cc / 100) << (4 * nch); ++nch;
    txt |= (u64)MSCNN_RENDER_GLYPH_DOT << (4 * nch); ++nch;
    txt |= (u64)((cc / 10) % 10) << (4 * nch); ++nch;
    txt |= (u64)(cc % 10) << (4 * nch); ++nch;
  }
  it.txt = txt;
  it.lw = nch * 6 * p.label_scale;
  const int lh = 8 * p.label_scale;
  it.lt = it.T - lh;
  if (it.lt < 0) it.lt = it.T;
  it.ll = it.L;
  if (it.ll + it.lw > w) { it.ll = w - it.lw; if (it.ll < 0) it.ll = 0; }
  *out = it;
  return true;
}

// the rounded mean of the source over the block of item `it` that holds (px, py), clipped to the box and the frame
__device__ __forceinline__ void render_mosaic(const RenderFrame& f, const RenderItem& it, int P, int px, int py, int v[3]) {
  const unsigned qx = ((unsigned)px - (unsigned)it.L) / (unsigned)P, qy = ((unsigned)py - (unsigned)it.T) / (unsigned)P;
  int bx0 = (int)((unsigned)it.L + qx * (unsigned)P), by0 = (int)((unsigned)it.T + qy * (unsigned)P);      // (<= px, py)
  int bx1 = bx0 + P - 1, by1 = by0 + P - 1;
  bx1 = bx1 > it.R ? it.R : bx1; bx1 = bx1 > f.w - 1 ? f.w - 1 : bx1;
  by1 = by1 > it.B ? it.B : by1; by1 = by1 > f.h - 1 ? f.h - 1 : by1;
  bx0 = bx0 < 0 ? 0 : bx0; by0 = by0 < 0 ? 0 : by0;
  int s0 = 0, s1 = 0, s2 = 0;
  for (int yy = by0; yy <= by1; ++yy) {
    const unsigned char* q = f.src + ((size_t)yy * f.w + bx0) * 3;
    for (int xx = bx0; xx <= bx1; ++xx, q += 3) { s0 += q[0]; s1 += q[1]; s2 += q[2]; }
  }
  const int n = (bx1 - bx0 + 1) * (by1 - by0 + 1);      // (>= 1: the pixel itself; <= 64 x 64)
  v[0] = (s0 + n / 2) / n; v[1] = (s1 + n / 2) / n; v[2] = (s2 + n / 2) / n;
}

// what pixel (px, py) takes from the n items of the list, in order
__device__ __forceinline__ void render_pixel(const mscnn_render_params& p, const RenderFrame& f, const RenderItem* list, int n,
                                             const unsigned char (*glyph)[7], int px, int py, int v[3]) {
  int first = 0;
  if (p.pixelate) {      // the last item that pixelates this pixel discards everything in front of it
    for (int i = n - 1; i > 0; --i) {
      const RenderItem& it = list[i];
      if (px >= it.L && px <= it.R && py >= it.T && py <= it.B) { first = i; break; }
    }
  }
  const int cell = 6 * p.label_scale, lh = 8 * p.label_scale;
  for (int i = first; i < n; ++i) {
    const RenderItem it = list[i];
    const int c0 = it.col & 255, c1 = (it.col >> 8) & 255, c2 = (it.col >> 16) & 255;
    if (px >= it.L && px <= it.R && py >= it.T && py <= it.B) {
      if (p.pixelate) render_mosaic(f, it, p.pixelate, px, py, v);                                             // (a)
      if (p.fill_alpha > 0) {                                                                                  // (b)
        v[0] = render_blend(v[0], c0, p.fill_alpha); v[1] = render_blend(v[1], c1, p.fill_alpha); v[2] = render_blend(v[2], c2, p.fill_alpha);
      }
      const unsigned th = (unsigned)p.thickness;                                                               // (c)
      if ((unsigned)px - (unsigned)it.L < th || (unsigned)it.R - (unsigned)px < th || (unsigned)py - (unsigned)it.T < th ||
          (unsigned)it.B - (unsigned)py < th) {
        v[0] = render_blend(v[0], c0, p.outline_alpha); v[1] = render_blend(v[1], c1, p.outline_alpha); v[2] = render_blend(v[2], c2, p.outline_alpha);
      }
    }
    if (it.lw > 0 && px >= it.ll && px < it.ll + it.lw && py >= it.lt && py < it.lt + lh) {                    // (d)
      const int dx = px - it.ll, dy = py - it.lt;
      const int ch = dx / cell, gx = (dx - ch * cell) / p.label_scale - 1, gy = dy / p.label_scale - 1;
      bool ink = false;
      if (gx >= 0 && gx < 5 && gy >= 0 && gy < 7) ink = (glyph[(it.txt >> (4 * ch)) & 15][gy] >> (4 - gx)) & 1;
      if (ink) { const int k = (it.col >> 24) & 1 ? 255 : 0; v[0] = k; v[1] = k; v[2] = k; }
      else { v[0] = c0; v[1] = c1; v[2] = c2; }
    }
  }
}

__global__ __launch_bounds__(kRenderThreads) void det_render_kernel(const RenderArgs a) {
  __shared__ RenderItem list[kRenderThreads];      // 10 KB
  __shared__ unsigned char glyph[16][7];           // (a text nibble indexes 16 rows: the last four stay blank)
  __shared__ int wsum[kRenderWaves];
  const RenderFrame& f = a.frame[blockIdx.z];
  const int tid = threadIdx.x;
  const int tiles_y = (f.h + kTileH - 1) / kTileH;
  if ((long long)blockIdx.x * kTileW >= f.w || (int)blockIdx.y >= tiles_y) return;      // (the grid is the chunk's largest frame's)
  if (tid < 16 * 7) glyph[tid / 7][tid % 7] = tid < MSCNN_RENDER_GLYPHS * 7 ? d_glyph[tid / 7][tid % 7] : 0;
  const int* hdr = reinterpret_cast<const int*>(a.pack);
  const double* rows = reinterpret_cast<const double*>(a.pack + a.dets_at);
  const int t = a.t0 + (int)blockIdx.z, K = a.num_slots;
  const bool want_id = a.ids != nullptr && (a.p.label >= 2 || a.p.color_by == 1);
  const int x0 = (int)blockIdx.x * kTileW, px = x0 + (tid & 63);
  const int x1 = x0 + kTileW - 1 < f.w - 1 ? x0 + kTileW - 1 : f.w - 1;
  const int lh = 8 * a.p.label_scale;
  for (int ty = blockIdx.y; ty < tiles_y; ty += gridDim.y) {      // (one round, unless the frame has more than 65535 tile rows)
    const int y0 = ty * kTileH, y1 = y0 + kTileH - 1 < f.h - 1 ? y0 + kTileH - 1 : f.h - 1;
    int v[kPixPerThread][3];
#pragma unroll
    for (int r = 0; r < kPixPerThread; ++r) {
      const int py = y0 + (tid >> 6) + kRenderWaves * r;
      v[r][0] = v[r][1] = v[r][2] = 0;
      if (px < f.w && py < f.h) {
        const unsigned char* q = f.src + ((size_t)py * f.w + px) * 3;
        v[r][0] = q[0]; v[r][1] = q[1]; v[r][2] = q[2];
      }
    }
    for (int k = 0; k < K; ++k) {
      long long off = 0;
      const int count = render_segment(hdr, K, t, k, a.cap, &off);      // (0 <= off, off + count <= cap: every thread alike)
      for (long long base = 0; base < count; base += kRenderThreads) {
        RenderItem it;
        bool hit = false;
        if (base + tid < count) {
          const size_t row = (size_t)off + (size_t)(count - 1 - (base + tid));      // descending: the best row is painted last
          hit = render_item(a.p, rows + 5 * row, want_id ? a.ids[row] : 0, k, f.h, f.w, &it);
          if (hit) {
            const bool box = it.L <= x1 && it.R >= x0 && it.T <= y1 && it.B >= y0;
            const bool lab = it.lw > 0 && it.ll <= x1 && it.ll + it.lw - 1 >= x0 && it.lt <= y1 && it.lt + lh - 1 >= y0;
            hit = box || lab;
          }
        }
        int n = 0;
        const int at = render_rank(hit, wsum, &n);      // (its first barrier also publishes the glyphs)
        if (hit) list[at] = it;
        __syncthreads();
        if (n > 0 && px < f.w) {
#pragma unroll
          for (int r = 0; r < kPixPerThread; ++r) {
            const int py = y0 + (tid >> 6) + kRenderWaves * r;
            if (py < f.h) render_pixel(a.p, f, list, n, glyph, px, py, v[r]);
          }
        }
        __syncthreads();      // (the list is free again)
      }
    }
#pragma unroll
    for (int r = 0; r < kPixPerThread; ++r) {
      const int py = y0 + (tid >> 6) + kRenderWaves * r;
      if (px < f.w && py < f.h) {
        unsigned char* q = f.dst + ((size_t)py * f.w + px) * 3;
        q[0] = (unsigned char)v[r][0]; q[1] = (unsigned char)v[r][1]; q[2] = (unsigned char)v[r][2];
      }
    }
  }
}

struct Span { uintptr_t lo, hi; int frame; bool dst; };
}  // namespace

using namespace mscnn;

extern "C" int mscnn_render_glyph_rows(int ch, unsigned char rows[7]) {
  MSCNN_REQUIRE(rows, "render_glyph_rows: null rows");
  const int code = ch >= '0' && ch <= '9' ? ch - '0' : ch == '.' ? MSCNN_RENDER_GLYPH_DOT : ch == ' ' ? MSCNN_RENDER_GLYPH_BLANK : -1;
  MSCNN_REQUIRE(code >= 0, "render_glyph_rows: character %d is none of '0' .. '9', '.' and ' '", ch);
  for (int r = 0; r < 7; ++r) rows[r] = h_glyph[code][r];
  return MSCNN_OK;
}

extern "C" int mscnn_render_detections_u8(const mscnn_render_params* p, const unsigned char* const* src_rgb, unsigned char* const* dst_rgb,
                                          const int* org_h, const int* org_w, int num_frames, int num_slots, const void* pack_dev, int cap,
                                          const int* track_ids_dev, void* stream) {
  const char* op = "render_detections";
  MSCNN_REQUIRE(p && src_rgb && dst_rgb && org_h && org_w && pack_dev, "%s: null pointer", op);
  const int T = num_frames, K = num_slots;
  MSCNN_REQUIRE(T >= 1, "%s: num_frames %d", op, T);
  MSCNN_REQUIRE(K >= 1, "%s: num_slots %d", op, K);
  MSCNN_REQUIRE(cap >= 1, "%s: cap %d", op, cap);
  MSCNN_REQUIRE((long)T * (long)K <= 0x7fffffffL && (long)T * (long)K * (long)cap <= 0x7fffffffL,
                "%s: %d frames x %d slots x %d pack rows is past 2^31 - 1", op, T, K, cap);
  for (int b = 0; b < T; ++b) {
    MSCNN_REQUIRE(org_h[b] > 0 && org_w[b] > 0 && org_h[b] <= (1 << 30) && org_w[b] <= (1 << 30),
                  "%s: frame %d has bad shape %d x %d (each inside [1, 2^30])", op, b, org_h[b], org_w[b]);
    MSCNN_REQUIRE(src_rgb[b], "%s: source frame %d is a null pointer", op, b);
    MSCNN_REQUIRE(dst_rgb[b], "%s: destination frame %d is a null pointer", op, b);
  }
  MSCNN_REQUIRE(p->thickness >= 0 && p->thickness <= 64, "%s: thickness %d is outside [0, 64]", op, p->thickness);
  MSCNN_REQUIRE(p->outline_alpha >= 0 && p->outline_alpha <= 256, "%s: outline_alpha %d is outside [0, 256]", op, p->outline_alpha);
  MSCNN_REQUIRE(p->fill_alpha >= 0 && p->fill_alpha <= 256, "%s: fill_alpha %d is outside [0, 256]", op, p->fill_alpha);
  MSCNN_REQUIRE(p->label >= 0 && p->label <= 3, "%s: label %d is outside [0, 3]", op, p->label);
  MSCNN_REQUIRE(p->label_scale >= 1 && p->label_scale <= 8, "%s: label_scale %d is outside [1, 8]", op, p->label_scale);
  MSCNN_REQUIRE(p->color_by == 0 || p->color_by == 1, "%s: color_by %d is neither 0 (slot) nor 1 (track id)", op, p->color_by);
  MSCNN_REQUIRE(p->pixelate == 0 || (p->pixelate >= 2 && p->pixelate <= 64), "%s: pixelate %d is neither 0 nor inside [2, 64]", op, p->pixelate);
  MSCNN_REQUIRE(p->num_colors >= 1 && p->num_colors <= 32, "%s: num_colors %d is outside [1, 32]", op, p->num_colors);
  MSCNN_REQUIRE(!(p->show_thr != p->show_thr), "%s: show_thr is NaN", op);
  MSCNN_REQUIRE(track_ids_dev || (p->label < 2 && p->color_by == 0), "%s: label %d, color_by %d need the track ids, track_ids_dev is null", op,
                p->label, p->color_by);
  MSCNN_REQUIRE(reinterpret_cast<uintptr_t>(pack_dev) % 16 == 0, "%s: pack_dev must be 16-byte aligned", op);
  MSCNN_REQUIRE(reinterpret_cast<uintptr_t>(track_ids_dev) % 4 == 0, "%s: track_ids_dev must be 4-byte aligned", op);
  // no dst frame may meet a src frame or another dst frame: sorted by their first byte, a span is held against the furthest end of
  // the dst spans and of the src spans in front of it
  std::vector<Span> spans(2 * (size_t)T);
  for (int b = 0; b < T; ++b) {
    const uintptr_t bytes = (uintptr_t)org_h[b] * (uintptr_t)org_w[b] * 3;
    const uintptr_t s = reinterpret_cast<uintptr_t>(src_rgb[b]), d = reinterpret_cast<uintptr_t>(dst_rgb[b]);
    spans[2 * (size_t)b] = Span{s, s + bytes, b, false};
    spans[2 * (size_t)b + 1] = Span{d, d + bytes, b, true};
  }
  std::sort(spans.begin(), spans.end(), [](const Span& x, const Span& y) { return x.lo < y.lo; });
  const Span* far_dst = nullptr;
  const Span* far_src = nullptr;
  for (const Span& s : spans) {
    MSCNN_REQUIRE(!(far_dst && far_dst->hi > s.lo), "%s: destination frame %d overlaps %s frame %d", op, far_dst->frame,
                  s.dst ? "destination" : "source", s.frame);
    MSCNN_REQUIRE(!(s.dst && far_src && far_src->hi > s.lo), "%s: destination frame %d overlaps source frame %d", op, s.frame, far_src->frame);
    const Span*& far = s.dst ? far_dst : far_src;
    if (!far || s.hi > far->hi) far = &s;
  }
  RenderArgs a = {};
  a.p = *p; a.num_slots = K; a.cap = cap;
  a.dets_at = mscnn_multi_pack_layout_of(T * K, cap).dets;
  a.pack = static_cast<const char*>(pack_dev); a.ids = track_ids_dev;
  hipStream_t st = as_stream(stream);
  for (int c0 = 0; c0 < T; c0 += kRenderFrames) {
    const int m = T - c0 < kRenderFrames ? T - c0 : kRenderFrames;
    long tx = 1, ty = 1;
    for (int s = 0; s < m; ++s) {
      a.frame[s] = RenderFrame{src_rgb[c0 + s], dst_rgb[c0 + s], org_h[c0 + s], org_w[c0 + s]};
      tx = std::max(tx, ((long)org_w[c0 + s] + kTileW - 1) / kTileW);
      ty = std::max(ty, ((long)org_h[c0 + s] + kTileH - 1) / kTileH);
    }
    a.t0 = c0;
    // the grid's y and z are bounded by 65535, x is not: a taller frame's workgroups take several tile rows each
    det_render_kernel<<<dim3((unsigned)tx, (unsigned)std::min(ty, 65535L), (unsigned)m), kRenderThreads, 0, st>>>(a);
    MSCNN_POST_LAUNCH();
  }
  return MSCNN_OK;
}
