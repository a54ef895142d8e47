// What det_device.h (the final stage's row transform) and proposals.hip (the proposal result) must agree on about BoxOutput's proposals_score rows
// [img x1 y1 x2 y2 score]: where an image's rows are, and which of them the scripts keep.  One definition each, so the two stages can
// not disagree about which ROI rows survive.
#pragma once
#include <hip/hip_runtime.h>

namespace mscnn_dev {

// first row whose image (column 0) is >= img, over [0, R): rows are grouped by image in ascending order (stride floats per row)
__device__ __forceinline__ int det_image_lower_bound(const float* __restrict__ props, int R, int img, int stride) {
  int lo = 0, hi = R;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (props[(size_t)mid * stride] < (float)img) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// run_mscnn_detection.m:82 on single values: sc = the proposal's score, pw = x2 - x1, ph = y2 - y1 (:78, no + 1).  A NaN score goes,
// -0.0 is zero, a negative extent stays.
__device__ __forceinline__ bool det_keep_proposal(float sc, float pw, float ph, float proposal_thr) {
  return sc >= proposal_thr && pw != 0 && ph != 0;
}

}  // namespace mscnn_dev
