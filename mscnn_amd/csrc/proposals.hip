// The proposal half of the scripts' result for gfx950: examples/kitti_car/run_mscnn_detection.m:75-91 (the same block in the
// caltech, kitti_ped_cyc and widerface drivers) for every image of a batched forward in one pass.
//   :78  w = x2 - x1, h = y2 - y1 in single (no + 1)
//   :82  keep score >= proposal_thr & w ~= 0 & h ~= 0 -- det_keep_proposal of det_rows.h, the predicate the final stage applies
//   :86  proposals = double(proposal_pred), THEN :87-90 x ./ ratios(2), w ./ ratios(2), y ./ ratios(1), h ./ ratios(1): double by
//        double (the final stage's det_row divides singles, because there the division comes before the double())
// Kept rows keep their input order.  Nothing is sorted, no workspace, no list-size limit.
#include <cmath>
#include <cstdint>
#include "common.h"
#include "det_rows.h"

namespace {
using namespace mscnn_dev;

constexpr int kPropThreads = 256;                                   // 4 waves: 256 rows per step
constexpr int kPropWaves = kPropThreads / 64;
constexpr int kPropImagesPerLaunch = MSCNN_PROPOSALS_IMAGES_PER_LAUNCH;   // the descs travel as kernel arguments (1.6 KB of the 4 KB)
struct PropImage { float proposal_thr; double ratio_h, ratio_w; };
struct PropArgs {
  const float* props; int R_all, num_images, cap, i0;              // i0: first image of this launch
  int* hdr; double* dets; int* ids;                                 // pack: header + table, rows, ROI row of each (mscnn_multi_pack_layout)
  PropImage img[kPropImagesPerLaunch];
};
static_assert(sizeof(PropArgs) <= 4096, "PropArgs travels as kernel arguments");

// One workgroup per image.  Steps of 256 rows: every wave ballots its 64 rows, the four popcounts meet in LDS, a kept row's place is
// the running base + the kept rows of the waves before its own + those of the lower lanes of its wave -- the input order, whatever
// the waves' timing.  The step's kept rows are gathered in LDS and leave as one contiguous run of doubles (a 40-byte row per lane
// would be five stores of 8 bytes at a 40-byte stride each).
__global__ __launch_bounds__(kPropThreads) void proposals_kernel(PropArgs a) {
  __shared__ int s_range[2];
  __shared__ int s_cnt[kPropWaves];
  __shared__ double s_row[kPropThreads * 5];
  __shared__ int s_src[kPropThreads];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = blockIdx.x, i = a.i0 + j;
  if (tid < 2) s_range[tid] = det_image_lower_bound(a.props, a.R_all, i + tid, 6);
  if (i == 0 && tid == 0) {
    a.hdr[0] = a.num_images; a.hdr[1] = a.R_all; a.hdr[2] = a.cap; a.hdr[3] = 0;
  }
  __syncthreads();
  const int row0 = s_range[0], rows = s_range[1] - s_range[0];
  const PropImage g = a.img[j];
  const float* __restrict__ p = a.props + 6 * (size_t)row0;
  const size_t slot = mscnn_multi_pack_slot(1, row0, 0, rows);      // the image's rows of the pack: [row0, row0 + rows)
  double* __restrict__ out = a.dets + 5 * slot;
  int* __restrict__ src = a.ids + slot;
  int base = 0;                                                     // rows kept so far (the same in every thread)
  for (int c0 = 0; c0 < rows; c0 += kPropThreads) {
    const int r = c0 + tid;
    bool keep = false;
    float px = 0.f, py = 0.f, pw = 0.f, ph = 0.f, sc = 0.f;
    if (r < rows) {
      // a row is 24 bytes at a multiple of 24: three 8-byte loads, adjacent lanes adjacent rows
      const float2* q = reinterpret_cast<const float2*>(p + 6 * (size_t)r);
      const float2 q0 = q[0], q1 = q[1], q2 = q[2];                 // [img x1] [y1 x2] [y2 score]
      px = q0.y; py = q1.x; pw = q1.y - q0.y; ph = q2.x - q1.x; sc = q2.y;
      keep = det_keep_proposal(sc, pw, ph, g.proposal_thr);
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_cnt[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < kPropWaves; ++w) {
      const int c = s_cnt[w];
      if (w < wave) before += c;
      total += c;
    }
    if (keep) {
      const int k = before + __popcll(m & ((1ull << lane) - 1ull));
      double* d = s_row + 5 * k;
      d[0] = (double)px / g.ratio_w; d[1] = (double)py / g.ratio_h;
      d[2] = (double)pw / g.ratio_w; d[3] = (double)ph / g.ratio_h;
      d[4] = (double)sc;
      s_src[k] = r;
    }
    __syncthreads();      // (also: every thread has read s_cnt before the next step writes it)
    for (int k = tid; k < 5 * total; k += kPropThreads) out[5 * (size_t)base + k] = s_row[k];
    if (tid < total) src[base + tid] = s_src[tid];
    base += total;
    // (the next step writes s_row / s_src behind its first barrier, which these reads have reached)
  }
  if (tid == 0) {
    int* ent = a.hdr + MSCNN_MULTI_PACK_WORDS * (size_t)(1 + i);
    ent[0] = base; ent[1] = rows; ent[2] = row0; ent[3] = 0;
  }
}
}  // namespace

using namespace mscnn;

extern "C" size_t mscnn_proposals_multi_pack_bytes(int num_images, int cap) { return mscnn_multi_pack_layout_of(num_images, cap).total; }

extern "C" int mscnn_proposals_multi_fwd(const mscnn_proposals_desc* desc, int num_images, const float* props, int R_all, void* pack_dev,
                                         int cap, void* stream) {
  MSCNN_REQUIRE(desc && props && pack_dev, "proposals_multi: null pointer");
  MSCNN_REQUIRE((reinterpret_cast<uintptr_t>(props) & 7) == 0 && (reinterpret_cast<uintptr_t>(pack_dev) & 15) == 0,
                "proposals_multi: props must be 8-byte and the pack 16-byte aligned");
  MSCNN_REQUIRE(num_images >= 1 && num_images <= (1 << 24), "proposals_multi: %d images (1 .. %d)", num_images, 1 << 24);
  MSCNN_REQUIRE(R_all >= 1, "proposals_multi: R_all = %d (BoxOutput emits at least one row)", R_all);
  MSCNN_REQUIRE(cap >= R_all, "proposals_multi: pack capacity %d < %d ROIs", cap, R_all);
  for (int i = 0; i < num_images; ++i) {
    MSCNN_REQUIRE(desc[i].ratio_h > 0 && desc[i].ratio_w > 0, "proposals_multi: image %d: ratios %g x %g (positive numbers)", i,
                  desc[i].ratio_h, desc[i].ratio_w);
    MSCNN_REQUIRE(!(desc[i].proposal_thr != desc[i].proposal_thr), "proposals_multi: image %d: proposal_thr is NaN", i);
  }
  hipStream_t st = as_stream(stream);
  PropArgs a = {};
  a.props = props; a.R_all = R_all; a.num_images = num_images; a.cap = cap;
  const mscnn_multi_pack_layout L = mscnn_multi_pack_layout_of(num_images, cap);
  char* pk = static_cast<char*>(pack_dev);
  a.hdr = reinterpret_cast<int*>(pk);
  a.dets = reinterpret_cast<double*>(pk + L.dets);
  a.ids = reinterpret_cast<int*>(pk + L.ids);
  for (int i0 = 0; i0 < num_images; i0 += kPropImagesPerLaunch) {
    const int ni = num_images - i0 < kPropImagesPerLaunch ? num_images - i0 : kPropImagesPerLaunch;
    a.i0 = i0;
    for (int j = 0; j < ni; ++j) a.img[j] = PropImage{desc[i0 + j].proposal_thr, desc[i0 + j].ratio_h, desc[i0 + j].ratio_w};
    proposals_kernel<<<ni, kPropThreads, 0, st>>>(a);
    MSCNN_POST_LAUNCH();
  }
  return MSCNN_OK;
}
