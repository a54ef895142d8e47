"""The numpy witness of the proposal half of the scripts' result, written from examples/kitti_car/run_mscnn_detection.m:75-91 (the
same block in the caltech, kitti_ped_cyc and widerface drivers).  No MATLAB here: this restatement is the check of the stage.

  :77  tmp = tmp(:,2:end)                          the image column goes          (single)
  :78  tmp(:,3) = tmp(:,3)-tmp(:,1); (:,4)-(:,2)   w, h: no + 1                   (single - single = single)
  :79  proposal_score = proposal_pred(:,end)
  :82  keep_id = find(proposal_score>=proposal_thr & proposal_pred(:,3)~=0 & proposal_pred(:,4)~=0)
                                                   single >= double compares in single; NaN >= x is false, -0 ~= 0 is false
  :86  proposals = double(proposal_pred)
  :87-90  columns 1, 3 ./ ratios(2), columns 2, 4 ./ ratios(1)                    (double ./ double)
"""
import numpy as np


def proposals_witness(rows6, proposal_thr, ratio_h, ratio_w, f32_division=False):
    """rows6: one image's rows [img x1 y1 x2 y2 score].  Returns (proposals [n, 5] float64 x y w h score, keep_id [n] int32: 0-based
    rows of rows6).  f32_division: the variant that divides BEFORE double() -- what the final stage's boxes do, NOT what :86-90 do;
    it exists so that a test can show its data tells the two apart."""
    tmp = np.array(rows6, np.float32).reshape(-1, 6)[:, 1:].copy()
    tmp[:, 2] = tmp[:, 2] - tmp[:, 0]
    tmp[:, 3] = tmp[:, 3] - tmp[:, 1]
    score = tmp[:, 4]
    with np.errstate(invalid="ignore"):
        keep = np.flatnonzero((score >= np.float32(proposal_thr)) & (tmp[:, 2] != 0) & (tmp[:, 3] != 0))
    pred = tmp[keep]
    if f32_division:
        rh, rw = np.float32(ratio_h), np.float32(ratio_w)
        pred = pred.copy()
        pred[:, 0] = pred[:, 0] / rw; pred[:, 2] = pred[:, 2] / rw
        pred[:, 1] = pred[:, 1] / rh; pred[:, 3] = pred[:, 3] / rh
        return pred.astype(np.float64), keep.astype(np.int32)
    out = pred.astype(np.float64)
    rh, rw = np.float64(ratio_h), np.float64(ratio_w)
    out[:, 0] = out[:, 0] / rw; out[:, 2] = out[:, 2] / rw
    out[:, 1] = out[:, 1] / rh; out[:, 3] = out[:, 3] / rh
    return out, keep.astype(np.int32)


def image_ranges(props6, num_images):
    """[(row0, rows)] per image of rows grouped by image in ascending order (an image without rows: where its rows would start)."""
    img = np.asarray(props6, np.float32).reshape(-1, 6)[:, 0]
    lo = np.searchsorted(img, np.arange(num_images, dtype=np.float32), "left")
    hi = np.searchsorted(img, np.arange(1, num_images + 1, dtype=np.float32), "left")
    return [(int(a), int(b - a)) for a, b in zip(lo, hi)]


def batch_witness(props6, images, f32_division=False):
    """images: one dict per image (ratios=(ratio_h, ratio_w), optionally proposal_thr).  Returns [(proposals, keep_id relative to
    row0, row0, rows)] per image."""
    props6 = np.asarray(props6, np.float32).reshape(-1, 6)
    out = []
    for (row0, rows), kw in zip(image_ranges(props6, len(images)), images):
        rh, rw = kw.get("ratios", (1.0, 1.0))
        p, k = proposals_witness(props6[row0:row0 + rows], kw.get("proposal_thr", -10.0), rh, rw, f32_division)
        out.append((p, k, row0, rows))
    return out


RATIOS = [(576 / 375.0, 1920 / 1242.0), (576 / 370.0, 1920 / 1224.0), (480 / 480.0, 640 / 600.0)]      # (H / orgH, W / orgW)


def synth_props(rows_per_image, seed):
    """proposals_score rows of a batch, grouped by image: boxes inside a 1920 x 576 frame, scores around proposal_thr = -10 (about
    half of the rows under it), some rows of zero width or height."""
    rng = np.random.default_rng(seed)
    parts = []
    for i, n in enumerate(rows_per_image):
        xy = rng.uniform(0, [1800, 500], (n, 2))
        wh = rng.uniform(4, 300, (n, 2))
        sc = rng.normal(-10.0, 3.0, (n, 1))      # (unsorted: the kept rows are scattered, which a sorted list would not do)
        parts.append(np.concatenate([np.full((n, 1), i), xy, xy + wh, sc], 1).astype(np.float32))
    props = np.concatenate(parts, 0) if parts else np.zeros((0, 6), np.float32)
    props[3::23, 3] = props[3::23, 1]      # x2 == x1
    props[7::31, 4] = props[7::31, 2]      # y2 == y1
    return props
