// The candidates of several forwards of an image, gathered before one NMS (mscnn_detections_candidates_*; the NMS itself is
// det_merge.hip / det_soft.hip).  `add` runs the rows of one forward through det_row -- the final stage's own row transform
// (det_device.h) -- applies the image's view in double and appends the survivors behind its list's count in row order.  One workgroup
// owns a list: no atomics on global memory, no workgroup waits on another, the order of a list is (order of the add calls, image, row)
// whatever the timing.
#include <cmath>
#include <vector>
#include "det_device.h"

namespace {
using namespace mscnn_dev;

// A launch carries up to kSegsPerLaunch ENTRIES, one per (image, slot) pair, sorted by list and then by image; workgroup q owns list
// `list[q]` and walks its entries [first[q], first[q + 1]) in turn, each behind the count the entries before it left.  The plain adds
// are the case of one image per list (list = image: one entry per workgroup), the views forms put the images of a frame into the
// frame's lists.  The count is read once and stored once, by this workgroup alone; a list whose entries do not fit one launch goes
// on in the next one, in stream order.
struct DetView { double off_x, off_y; int flip_x, on; };      // on = 0: view == NULL, the box leaves as det_row returned it
struct DetCandArgs {
  int R_all, classes_per_source, cand_cap, num_segs, pass, num_blocks;      // num_segs: lists of the cand buffer
  char* cand;
  DetNms nms;
  DetSource src[kCascadeMaxOutputs];
  DetSeg seg[kSegsPerLaunch];
  DetView view[kSegsPerLaunch];
  int img[kSegsPerLaunch], slot[kSegsPerLaunch];      // entry -> its image of the batch and its slot of the image
  int list[kSegsPerLaunch], first[kSegsPerLaunch + 1];      // workgroup -> its list and its entries
};
static_assert(sizeof(DetCandArgs) <= 4096, "DetCandArgs travels as kernel arguments");
constexpr int kCandThreads = 256;

// an entry's rows in steps of 256: a kept row's place = the list's count + the kept rows of the waves before its own + those of the
// lower lanes of its wave (ballot / popcount, as proposals.hip)
template <bool kThr>
__device__ __forceinline__ void det_cand_add(const DetCandArgs& a) {
  const int q = blockIdx.x, s = a.list[q], tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const DetCand c = det_cand_of(a.cand, a.num_segs, a.cand_cap);
  __shared__ int s_range[2];
  __shared__ int s_base;
  __shared__ int s_cnt[kCandThreads / 64];
  if (tid == 0) s_base = c.cnt[CAND_WORDS * (size_t)s + CAND_WANTED];
  __syncthreads();
  int base = s_base;
  const size_t list = (size_t)s * (size_t)a.cand_cap;
  for (int e = a.first[q]; e < a.first[q + 1]; ++e) {
    const DetSource& t = a.src[a.slot[e] / a.classes_per_source];
    __syncthreads();      // (every thread has read the range of the entry before)
    if (tid < 2) s_range[tid] = det_image_lower_bound(t.props, a.R_all, a.img[e] + tid, t.cascade ? 5 : 6);
    __syncthreads();
    const int row0 = s_range[0], rows = s_range[1] - s_range[0];
    const DetArgs d = det_args_of(t, a.seg[e], row0, rows, a.nms);
    const DetView v = a.view[e];
    for (int r0 = 0; r0 < rows; r0 += kCandThreads) {
      const int r = r0 + tid;
      DetBox b;
      float prob = 0.f;
      bool keep = false;
      if (r < rows) keep = det_row<kThr>(d, r, &b, &prob);
      const u64 m = __ballot(keep);
      if (lane == 0) s_cnt[wave] = __popcll(m);
      __syncthreads();
      int before = 0, total = 0;
      for (int w = 0; w < kCandThreads / 64; ++w) {
        if (w < wave) before += s_cnt[w];
        total += s_cnt[w];
      }
      if (keep) {
        const long pos = (long)base + before + __popcll(m & ((1ull << lane) - 1ull));
        if (pos < (long)a.cand_cap) {                     // (past the cap nothing is stored: the count below says how many wanted in)
          if (v.on) {
            if (v.flip_x) b.x = (double)d.org_w - (b.x + b.w);
            b.x = b.x + v.off_x;
            b.y = b.y + v.off_y;
          }
          c.box[list + pos] = b;
          c.prob[list + pos] = prob;
          c.tag[list + pos] = (a.pass << 24) | (row0 + r);
        }
      }
      const long nb = (long)base + total;
      base = nb > 0x7fffffffL ? 0x7fffffff : (int)nb;
      __syncthreads();      // (every thread has read s_cnt before the next step writes it)
    }
  }
  if (tid == 0) {
    c.cnt[CAND_WORDS * (size_t)s + CAND_WANTED] = base;
    if (base > a.cand_cap) c.cnt[CAND_WORDS * (size_t)s + CAND_OVER] = 1;
  }
}
__global__ __launch_bounds__(kCandThreads) void det_cand_add_list_kernel(DetCandArgs a) { det_cand_add<false>(a); }
__global__ __launch_bounds__(kCandThreads) void det_cand_add_list_thr_kernel(DetCandArgs a) { det_cand_add<true>(a); }
}  // namespace

using namespace mscnn;

extern "C" size_t mscnn_detections_candidates_bytes(int num_segments, int cand_cap) {
  return cand_shape_ok(num_segments, cand_cap) ? det_cand_bytes(num_segments, cand_cap) : 0;
}

extern "C" int mscnn_detections_candidates_reset(void* cand, int num_segments, int cand_cap, void* stream) {
  MSCNN_REQUIRE(cand, "detections_candidates_reset: null pointer");
  MSCNN_REQUIRE(num_segments >= 1, "detections_candidates_reset: %d segments", num_segments);
  MSCNN_REQUIRE(cand_cap >= 1, "detections_candidates_reset: cand_cap %d", cand_cap);
  MSCNN_REQUIRE(cand_shape_ok(num_segments, cand_cap), "detections_candidates_reset: %d segments x %d slots is past 2^31 - 1", num_segments,
                cand_cap);
  MSCNN_REQUIRE_ALIGNED(cand, 16, "detections_candidates_reset: cand");
  MSCNN_HIP_TRY(hipMemsetAsync(cand, 0, (size_t)num_segments * CAND_WORDS * sizeof(int), as_stream(stream)));
  return MSCNN_OK;
}

// Everything the add calls refuse alike, then the entries (image, slot) sorted by list, then slot, then image ascending: 32 per
// launch, one workgroup per list of a launch.  list_of == NULL: the plain forms, image b into list b (num_lists = num_images).
static int det_cand_launch(const char* name, const DetSource* src, int num_sources, const mscnn_detections_desc* desc,
                           const mscnn_detections_view* view, float det_thr, const mscnn_nms_params& nms, int pass, int num_images, int C,
                           int R_all, void* cand, int cand_cap, void* stream, const int* list_of, int num_lists) {
  const int K = num_sources * C;
  MSCNN_REQUIRE((long)num_images * K <= (long)(1 << 24), "%s: %d images x %d slots", name, num_images, K);
  MSCNN_REQUIRE(!list_of || (long)num_lists * K <= (long)(1 << 24), "%s: %d lists x %d slots", name, num_lists, K);
  if (!list_of) num_lists = num_images;
  const int S = num_lists * K;
  MSCNN_REQUIRE(cand_cap >= 1, "%s: cand_cap %d", name, cand_cap);
  MSCNN_REQUIRE(cand_shape_ok(S, cand_cap), "%s: %d segments x %d slots is past 2^31 - 1", name, S, cand_cap);
  MSCNN_REQUIRE_ALIGNED(cand, 16, "detections_candidates: cand");
  MSCNN_REQUIRE(pass >= 0 && pass <= 127, "%s: pass %d (0 .. 127: the tag is (pass << 24) | row)", name, pass);
  MSCNN_REQUIRE(R_all >= 1, "%s: R_all = %d (BoxOutput emits at least one row)", name, R_all);
  MSCNN_REQUIRE(R_all < (1 << 24), "%s: R_all = %d rows do not fit the tag's 24 row bits", name, R_all);
  for (int s = 0; s < num_images * K; ++s) {
    MSCNN_REQUIRE(desc[s].ratio_h > 0 && desc[s].ratio_w > 0, "%s: segment %d: ratios %g x %g (positive numbers)", name, s, desc[s].ratio_h,
                  desc[s].ratio_w);
  }
  for (int i = 0; view && i < num_images; ++i) {
    MSCNN_REQUIRE(std::isfinite(view[i].off_x) && std::isfinite(view[i].off_y), "%s: image %d: view offset (%g, %g) is not finite", name, i,
                  view[i].off_x, view[i].off_y);
    MSCNN_REQUIRE(view[i].flip_x == 0 || view[i].flip_x == 1, "%s: image %d: flip_x %d (0 or 1)", name, i, view[i].flip_x);
  }
  hipStream_t st = as_stream(stream);
  DetCandArgs a = {};
  a.R_all = R_all; a.classes_per_source = C; a.cand_cap = cand_cap; a.num_segs = S; a.pass = pass;
  a.cand = static_cast<char*>(cand);
  a.nms = det_nms_of(nms);
  for (int o = 0; o < num_sources; ++o) a.src[o] = src[o];
  // the images grouped by list, ascending inside a list (a counting sort in one flat array): order[start[f] .. start[f + 1]) go to list f
  std::vector<int> start((size_t)num_lists + 2 + num_images, 0);
  int* order = start.data() + num_lists + 2;
  for (int b = 0; b < num_images; ++b) ++start[(list_of ? list_of[b] : b) + 2];
  for (int f = 0; f < num_lists; ++f) start[f + 2] += start[f + 1];      // start[f + 1]: the first place of list f ...
  for (int b = 0; b < num_images; ++b) order[start[(list_of ? list_of[b] : b) + 1]++] = b;      // ... and now the one behind its last
  int n = 0, last_list = -1;
  auto flush = [&]() -> int {
    if (n == 0) return MSCNN_OK;
    a.first[a.num_blocks] = n;
    if (nms_has_thr(nms)) det_cand_add_list_thr_kernel<<<a.num_blocks, kCandThreads, 0, st>>>(a);
    else det_cand_add_list_kernel<<<a.num_blocks, kCandThreads, 0, st>>>(a);
    MSCNN_POST_LAUNCH();
    n = 0; a.num_blocks = 0; last_list = -1;
    return MSCNN_OK;
  };
  for (int f = 0; f < num_lists; ++f) {
    for (int k = 0; k < K; ++k) {
      for (int i = start[f]; i < start[f + 1]; ++i) {
        const int b = order[i], s = f * K + k;
        if (s != last_list) { a.list[a.num_blocks] = s; a.first[a.num_blocks] = n; ++a.num_blocks; last_list = s; }
        a.seg[n] = det_seg_of(desc[b * K + k], src[0].cascade, det_thr);
        a.view[n] = view ? DetView{view[b].off_x, view[b].off_y, view[b].flip_x, 1} : DetView{0.0, 0.0, 0, 0};
        a.img[n] = b; a.slot[n] = k;
        if (++n == kSegsPerLaunch) { if (int rc = flush()) return rc; }
      }
    }
  }
  return flush();
}

// what list_of must be in the views forms (checked in front of everything the plain forms check)
static int det_list_of_checked(const char* name, const int* list_of, int num_images, int num_lists) {
  MSCNN_REQUIRE(list_of, "%s: null pointer (list_of)", name);
  MSCNN_REQUIRE(num_lists >= 1, "%s: num_lists %d < 1", name, num_lists);
  for (int b = 0; b < num_images; ++b)
    MSCNN_REQUIRE(list_of[b] >= 0 && list_of[b] < num_lists, "%s: image %d: list_of %d outside [0, %d)", name, b, list_of[b], num_lists);
  return MSCNN_OK;
}

// the plain add and its views form (list_of != NULL)
static int det_cand_add_plain(const char* name, const mscnn_detections_desc* desc, const mscnn_detections_view* view, const int* list_of,
                              int num_lists, const mscnn_nms_params* nms_in, int pass, int num_images, int num_classes,
                              const float* bbox_pred, const float* cls_pred, const float* props, int R_all, void* cand, int cand_cap,
                              void* stream) {
  mscnn_nms_params nms;
  if (int rc = mscnn_nms_params_resolve(nms_in, &nms)) return rc;
  MSCNN_REQUIRE(desc && cand && bbox_pred && cls_pred && props, "%s: null pointer", name);
  MSCNN_REQUIRE(num_images >= 1 && num_classes >= 1, "%s: %d images x %d classes", name, num_images, num_classes);
  MSCNN_REQUIRE((long)num_images * num_classes <= (long)(1 << 24), "%s: %d images x %d classes", name, num_images, num_classes);
  DetSource src;
  if (int rc = det_plain_source(name, desc, num_images * num_classes, bbox_pred, cls_pred, props, &src)) return rc;
  return det_cand_launch(name, &src, 1, desc, view, 0.f, nms, pass, num_images, num_classes, R_all, cand, cand_cap, stream, list_of, num_lists);
}

extern "C" int mscnn_detections_candidates_add(const mscnn_detections_desc* desc, const mscnn_detections_view* view,
                                               const mscnn_nms_params* nms_in, int pass, int num_images, int num_classes,
                                               const float* bbox_pred, const float* cls_pred, const float* props, int R_all, void* cand,
                                               int cand_cap, void* stream) {
  return det_cand_add_plain("detections_candidates_add", desc, view, nullptr, 0, nms_in, pass, num_images, num_classes, bbox_pred, cls_pred,
                            props, R_all, cand, cand_cap, stream);
}

extern "C" int mscnn_detections_candidates_add_views(const mscnn_detections_desc* desc, const mscnn_detections_view* view, const int* list_of,
                                                     const mscnn_nms_params* nms_in, int pass, int num_images, int num_lists, int num_classes,
                                                     const float* bbox_pred, const float* cls_pred, const float* props, int R_all, void* cand,
                                                     int cand_cap, void* stream) {
  const char* name = "detections_candidates_add_views";
  MSCNN_REQUIRE(num_images >= 1 && num_classes >= 1, "%s: %d images x %d classes", name, num_images, num_classes);
  if (int rc = det_list_of_checked(name, list_of, num_images, num_lists)) return rc;
  return det_cand_add_plain(name, desc, view, list_of, num_lists, nms_in, pass, num_images, num_classes, bbox_pred, cls_pred, props, R_all, cand,
                            cand_cap, stream);
}

// the cascade add and its views form (list_of != NULL)
static int det_cand_add_cascade(const char* name, const mscnn_detections_desc* desc, const mscnn_detections_view* view, const int* list_of,
                                int num_lists, float det_thr, const mscnn_nms_params* nms_in, int pass, int num_images, int num_outputs,
                                int num_classes, const mscnn_cascade_output* outputs, int R_all, void* cand, int cand_cap, void* stream) {
  mscnn_nms_params nms;
  if (int rc = mscnn_nms_params_resolve(nms_in, &nms)) return rc;
  MSCNN_REQUIRE(nms.det_thr == 0.f, "%s: nms params det_thr %g is the plain stage's: the cascade stage takes its det_thr as an argument", name,
                (double)nms.det_thr);
  MSCNN_REQUIRE(num_outputs >= 1 && num_outputs <= kCascadeMaxOutputs, "%s: %d cascade outputs (1 .. %d)", name, num_outputs,
                kCascadeMaxOutputs);
  MSCNN_REQUIRE(desc && outputs && cand, "%s: null pointer", name);
  MSCNN_REQUIRE(num_images >= 1 && num_classes >= 1, "%s: %d images x %d classes", name, num_images, num_classes);
  DetSource src[kCascadeMaxOutputs];
  if (int rc = det_cascade_sources(name, desc, num_images, num_outputs, num_classes, outputs, src)) return rc;
  return det_cand_launch(name, src, num_outputs, desc, view, det_thr, nms, pass, num_images, num_classes, R_all, cand, cand_cap, stream, list_of,
                         num_lists);
}

extern "C" int mscnn_detections_candidates_cascade_add(const mscnn_detections_desc* desc, const mscnn_detections_view* view, float det_thr,
                                                       const mscnn_nms_params* nms_in, int pass, int num_images, int num_outputs,
                                                       int num_classes, const mscnn_cascade_output* outputs, int R_all, void* cand,
                                                       int cand_cap, void* stream) {
  return det_cand_add_cascade("detections_candidates_cascade_add", desc, view, nullptr, 0, det_thr, nms_in, pass, num_images, num_outputs,
                              num_classes, outputs, R_all, cand, cand_cap, stream);
}

extern "C" int mscnn_detections_candidates_cascade_add_views(const mscnn_detections_desc* desc, const mscnn_detections_view* view,
                                                             const int* list_of, float det_thr, const mscnn_nms_params* nms_in, int pass,
                                                             int num_images, int num_lists, int num_outputs, int num_classes,
                                                             const mscnn_cascade_output* outputs, int R_all, void* cand, int cand_cap,
                                                             void* stream) {
  const char* name = "detections_candidates_cascade_add_views";
  MSCNN_REQUIRE(num_images >= 1 && num_classes >= 1, "%s: %d images x %d classes", name, num_images, num_classes);
  if (int rc = det_list_of_checked(name, list_of, num_images, num_lists)) return rc;
  return det_cand_add_cascade(name, desc, view, list_of, num_lists, det_thr, nms_in, pass, num_images, num_outputs, num_classes, outputs, R_all,
                              cand, cand_cap, stream);
}
