"""A numpy restatement of the merged final stage (mscnn_detections_candidates_* + mscnn_detections_merge_fwd, Net.detect_merge_*):
several forwards of an image, one NMS.  No pin on the reference -- its scripts run one forward per image -- so this is the check.

Per pass the rows go through the scripts' row transform WITHOUT the NMS:
  * plain stage: run_mscnn_detection.m:75-113 restated below, the statements of tests/witness.final_stage up to its bbNms call
    (that function is left as it is), with exp(single) as C's expf -- the final stage restates libm's expf bit for bit, numpy's own
    float32 exp may differ from it in the last place;
  * cascade stage: run_cascademscnn.m:96-124 restated below, one statement per line, single until `double(...)`;
then bbNms's thr (bbNms.m:85, strict) and the plain det_thr (widerface/run_mscnn_detection.m:139-143), the pass's view in float64,
concatenation in add order, a stable descending sort (ties: the earlier candidate) and nms_witness.nms_max.

TEST INFRASTRUCTURE ONLY."""
import ctypes
import ctypes.util

import numpy as np

import nms_witness

f32 = np.float32


_libm = None


def expf(x):
    """C's expf on every element of a single array: the scripts' exp(single) as the final stage restates it (libm's expf bit for
    bit; numpy's own float32 exp may differ from it in the last place, which a bit-for-bit comparison can not accept)."""
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        _libm.expf.restype = ctypes.c_float
        _libm.expf.argtypes = [ctypes.c_float]
    x = np.asarray(x, f32)
    return np.array([_libm.expf(float(v)) for v in x.ravel()], f32).reshape(x.shape)


def plain_rows(bbox_pred, cls_pred, props, cls_id, thr=None, det_thr=0.0, bbox_means=(0, 0, 0, 0), bbox_stds=(0.1, 0.1, 0.2, 0.2),
               proposal_thr=-10.0, ratios=(1.0, 1.0), org_hw=(375, 1242), exp=None):
    """run_mscnn_detection.m:75-113 for ONE image of one forward and one class, without bbNms: the rows that reach the NMS, in row
    order: (rows [n, 5] float64 [x y w h prob], ids [n] = row of the blobs handed in).  The statements of witness.final_stage, one
    MATLAB statement per line, with exp(single) as C's expf (exp: another exp on single arrays, for callers who time this function
    and need no bit-exactness: tools/bench_final_stage.py --merge hands in numpy's)."""
    exp = expf if exp is None else exp
    tmp = np.asarray(props, f32).reshape(-1, 6)[:, 1:].copy()                                  # :76-77 tmp(:,2:end)
    if len(tmp) == 0:
        return np.zeros((0, 5)), np.zeros(0, np.int32)
    bbox_preds = np.asarray(bbox_pred, f32).reshape(len(tmp), -1)
    cls_pred = np.asarray(cls_pred, f32).reshape(len(tmp), -1)
    tmp[:, 2] = tmp[:, 2] - tmp[:, 0]                                                          # :78
    tmp[:, 3] = tmp[:, 3] - tmp[:, 1]
    proposal_pred = tmp
    keep_id = np.flatnonzero((proposal_pred[:, 4] >= f32(proposal_thr)) & (proposal_pred[:, 2] != 0) & (proposal_pred[:, 3] != 0))   # :82
    proposal_pred, bbox_preds, cls_pred = proposal_pred[keep_id], bbox_preds[keep_id], cls_pred[keep_id]
    bbox = bbox_preds[:, cls_id * 4 - 4:cls_id * 4]                                            # :95
    bbox = bbox * np.asarray(bbox_stds, f32)[None, :]
    bbox = bbox + np.asarray(bbox_means, f32)[None, :]
    exp_score = exp(cls_pred)                                                                 # :101
    sum_exp_score = np.zeros(len(cls_pred), f32)
    for c in range(cls_pred.shape[1]):                                                         # :102 sum(exp_score,2), left to right
        sum_exp_score = sum_exp_score + exp_score[:, c]
    prob = exp_score[:, cls_id - 1] / sum_exp_score
    ctr_x = proposal_pred[:, 0] + f32(0.5) * proposal_pred[:, 2]
    ctr_y = proposal_pred[:, 1] + f32(0.5) * proposal_pred[:, 3]
    tx = bbox[:, 0] * proposal_pred[:, 2] + ctr_x
    ty = bbox[:, 1] * proposal_pred[:, 3] + ctr_y
    tw = proposal_pred[:, 2] * exp(bbox[:, 2])
    th = proposal_pred[:, 3] * exp(bbox[:, 3])
    tx = tx - tw / f32(2); ty = ty - th / f32(2)
    tx = tx / f32(ratios[1]); tw = tw / f32(ratios[1])                                         # single ./ double -> single
    ty = ty / f32(ratios[0]); th = th / f32(ratios[0])
    tx = np.maximum(f32(0), tx); ty = np.maximum(f32(0), ty)
    tw = np.minimum(tw, f32(org_hw[1]) - tx); th = np.minimum(th, f32(org_hw[0]) - ty)
    bbset = np.stack([tx, ty, tw, th, prob], 1).astype(np.float64)                             # double([tx ty tw th prob])
    return _thresholds(bbset, keep_id.astype(np.int32), thr, det_thr)


def cascade_rows(boxes, cls_prob, props, cls_id, ratios=(1.0, 1.0), org_hw=(375, 1242), det_thr=0.0, thr=None):
    """run_cascademscnn.m:96-124 for one image, one cascade output and one class, without bbNms."""
    tmp = np.asarray(boxes, f32).reshape(-1, 5)[:, 1:].copy()                        # :96-97
    if len(tmp) == 0:
        return np.zeros((0, 5)), np.zeros(0, np.int32)
    tmp[:, [0, 2]] = tmp[:, [0, 2]] / f32(ratios[1])                                 # :98 (single ./ double -> single)
    tmp[:, [1, 3]] = tmp[:, [1, 3]] / f32(ratios[0])                                 # :99
    tmp[:, [0, 1]] = np.maximum(f32(0), tmp[:, [0, 1]])                              # :101
    tmp[:, 2] = np.minimum(tmp[:, 2], f32(org_hw[1])); tmp[:, 3] = np.minimum(tmp[:, 3], f32(org_hw[0]))   # :102
    tmp[:, [2, 3]] = tmp[:, [2, 3]] - tmp[:, [0, 1]] + f32(1)                        # :103
    output_bboxs = tmp.astype(np.float64)                                            # :104
    cls_prob = np.asarray(cls_prob, f32).reshape(len(tmp), -1)                       # :106-107
    p = np.asarray(props, f32).reshape(-1, 5)[:, 1:].copy()                          # :109-110
    p[:, [2, 3]] = p[:, [2, 3]] - p[:, [0, 1]] + f32(1)                              # :111
    keep_id = np.flatnonzero((p[:, 2] != 0) & (p[:, 3] != 0))                        # :114
    prob = cls_prob[keep_id, cls_id - 1]                                             # :120
    bbset = np.concatenate([output_bboxs[keep_id], prob[:, None].astype(np.float64)], 1)      # :121
    if det_thr > 0:                                                                  # :122-124
        k = prob >= f32(det_thr)
        bbset, keep_id = bbset[k], keep_id[k]
    return _thresholds(bbset, keep_id.astype(np.int32), thr, 0.0)


def _thresholds(rows, ids, thr, det_thr):
    keep = rows[:, 4] > (-np.inf if thr is None else thr)                            # bbNms.m:85 (NaN drops out)
    if det_thr > 0:
        keep &= rows[:, 4].astype(f32) >= f32(det_thr)                               # widerface/run_mscnn_detection.m:139-143
    return rows[keep], ids[keep].astype(np.int32)


def apply_view(rows, org_w, view=None):
    """The view of a pass, in float64, on [x y w h prob] rows: view None (the identity) or (off_x, off_y, flip_x).
    org_w: the float the rows were clipped against (single(orgW))."""
    rows = np.array(rows, np.float64).reshape(-1, 5)
    if view is None:
        return rows
    off_x, off_y, flip_x = view
    x = rows[:, 0]
    if flip_x:
        x = np.float64(f32(org_w)) - (x + rows[:, 2])
    rows[:, 0] = x + np.float64(off_x)
    rows[:, 1] = rows[:, 1] + np.float64(off_y)
    return rows


def merge(passes, overlap=0.5, type="maxg", ovr_dnm="union"):
    """passes: [(rows [n, 5] float64 in original-image coordinates, row ids [n])] in add order, for ONE segment.
    Returns (dets [D, 5], pass [D], row [D], candidates)."""
    rows = np.concatenate([np.asarray(r, np.float64).reshape(-1, 5) for r, _ in passes]) if passes else np.zeros((0, 5))
    pas = np.concatenate([np.full(len(i), k, np.int32) for k, (_, i) in enumerate(passes)]) if passes else np.zeros(0, np.int32)
    ids = np.concatenate([np.asarray(i, np.int32) for _, i in passes]) if passes else np.zeros(0, np.int32)
    srt, order = nms_witness.sort_rows(rows)                  # stable: a tie goes to the earlier candidate
    keep = nms_witness.nms_max(srt, overlap, greedy=(type == "maxg"), ovr_dnm=ovr_dnm)
    return srt[keep], pas[order][keep], ids[order][keep], len(rows)


def cross_pass_facts(passes, overlap=0.5, type="maxg", ovr_dnm="union"):
    """What a multi-pass case must show on the witness's own result before anything is compared with it: (a later pass's box is
    suppressed by an earlier pass's, an earlier pass's by a later pass's, the set of passes with a survivor).  'Suppressed by':
    the overlap of the pair is over the threshold, the suppressor comes first in the sort and (greedy) is itself kept."""
    rows = np.concatenate([np.asarray(r, np.float64).reshape(-1, 5) for r, _ in passes])
    pas = np.concatenate([np.full(len(i), k, np.int32) for k, (_, i) in enumerate(passes)])
    srt, order = nms_witness.sort_rows(rows)
    pas = pas[order]
    greedy = type == "maxg"
    keep = nms_witness.nms_max(srt, overlap, greedy=greedy, ovr_dnm=ovr_dnm)
    o = nms_witness.overlaps(srt, ovr_dnm) > overlap
    later_by_earlier = earlier_by_later = False
    for i in range(len(srt)):
        if greedy and not keep[i]:
            continue
        hit = np.flatnonzero(o[i])
        later_by_earlier |= bool(np.any(pas[hit] > pas[i]))
        earlier_by_later |= bool(np.any(pas[hit] < pas[i]))
    return later_by_earlier, earlier_by_later, set(pas[keep].tolist())
