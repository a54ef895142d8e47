"""Two witnesses of Soft-NMS over the merged candidates (mscnn_detections_merge_soft_fwd, Net.set_soft_nms; Bodla et al., 2017), on
top of merge_witness and vote_witness.candidates_of.  No pin on the reference -- its scripts neither merge nor decay a score -- so
these are the check.

  * soft(): a float64 numpy restatement of the op's contract (include/mscnn_hip.h), statement for statement: pick the live candidate
    with the largest score (a NaN ranks below every number; equal scores: the lowest slot), stop below score_thr, emit, decay every
    live candidate by its union overlap with the pick -- the vote's overlap statements, each operation rounded.  The LINEAR method
    is compared bit for bit (IEEE operations only); the GAUSSIAN one calls exp, numpy's here and OCML's on the device, and is
    compared within a derived allowance.  It also returns min_gap: the smallest relative gap any pick saw between the picked score
    and the runner-up's, or between the picked score and score_thr -- how far the inputs are from a pick that a last-bit difference
    could turn.
  * soft_exact(): the linear method in exact rational arithmetic (fractions.Fraction): the exact score of every pick, what the
    float witness itself is measured against.

TEST INFRASTRUCTURE ONLY."""
from fractions import Fraction

import numpy as np

import merge_witness as mw
from vote_witness import candidates_of

LINEAR, GAUSSIAN = 1, 2
METHODS = {"linear": LINEAR, "gaussian": GAUSSIAN}


def decay_ratio(A, B):
    """(hit, r) of the picked box A = [x y w h] against the boxes B [n, >= 4]: the op's statements one per line, all in float64.
    hit: the op reached the ratio (it skips a pair on iw <= 0, then on ih <= 0) and the ratio is no NaN."""
    A = np.asarray(A, np.float64)
    B = np.asarray(B, np.float64)
    as_a = A[2] * A[3]
    xe_a = A[0] + A[2]
    ye_a = A[1] + A[3]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        iw = np.fmin(xe_a, B[:, 0] + B[:, 2]) - np.fmax(A[0], B[:, 0])
        ih = np.fmin(ye_a, B[:, 1] + B[:, 3]) - np.fmax(A[1], B[:, 1])
        o = iw * ih
        u = as_a + B[:, 2] * B[:, 3] - o
        r = o / u
    return ~(iw <= 0) & ~(ih <= 0) & ~np.isnan(r), r


def rank_key(s):
    """The score as the argmax ranks it: a NaN below every number."""
    return np.where(np.isnan(s), -np.inf, s)


def soft(cand, method, overlap=0.5, sigma=0.5, score_thr=0.001, max_out=0):
    """One segment: cand [n, 5] float64 [x y w h prob] in slot order.  Returns (dets [D, 5] with the score at its pick, slots [D] in
    pick order, decays: how many score updates changed a score, min_gap)."""
    cand = np.asarray(cand, np.float64).reshape(-1, 5)
    n = len(cand)
    s = cand[:, 4].astype(np.float32).astype(np.float64)      # (double)prob_j: the list holds the prob as a float
    live = np.ones(n, bool)
    dets, slots, decays, min_gap = [], [], 0, np.inf
    score_thr, sigma, overlap = np.float64(score_thr), np.float64(sigma), np.float64(overlap)
    while live.any() and not (max_out > 0 and len(dets) == max_out):
        key = np.where(live, rank_key(s), -np.inf)
        idx = np.flatnonzero(live)
        m = int(idx[np.argmax(key[idx])])                      # (argmax: the first of equals, the lowest slot)
        with np.errstate(divide="ignore", invalid="ignore"):
            others = key[idx[idx != m]]
            gaps = [abs(s[m] - score_thr) / abs(s[m])]
            if len(others):
                gaps.append((s[m] - others.max()) / abs(s[m]))
            g = np.min(gaps)
            min_gap = min(min_gap, 0.0 if np.isnan(g) else float(g))
        if not (s[m] >= score_thr):
            break
        dets.append(np.concatenate([cand[m, :4], [s[m]]]))
        slots.append(m)
        live[m] = False
        hit, r = decay_ratio(cand[m, :4], cand)
        if method == LINEAR:
            upd = live & hit & (r > overlap)
            new = s * (1.0 - r)
        else:
            upd = live & hit
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                new = s * np.exp(-(r * r) / sigma)
        with np.errstate(invalid="ignore"):
            decays += int(np.count_nonzero(upd & (new != s)))
        s = np.where(upd, new, s)
    return np.array(dets, np.float64).reshape(-1, 5), np.array(slots, np.int64), decays, min_gap


def soft_segment(passes, method, overlap=0.5, sigma=0.5, score_thr=0.001, max_out=0):
    """One segment from its passes (merge_witness.merge's argument): (dets, pass [D], row [D], candidates, slots, decays, min_gap)."""
    cand, cand_pass = candidates_of(passes)
    ids = np.concatenate([np.asarray(i, np.int32) for _, i in passes]) if passes else np.zeros(0, np.int32)
    dets, slots, decays, min_gap = soft(cand, method, overlap, sigma, score_thr, max_out)
    return dets, cand_pass[slots], ids[slots], len(cand), slots, decays, min_gap


def soft_exact(cand, overlap=0.5, score_thr=0.001, max_out=0):
    """The linear method in exact rationals (every float64 is one): (slots in pick order, the exact score of every pick, the
    relative error bound of the float64 score of every pick).
    The bound, for boxes whose coordinates are small integers -- then iw, ih, o and u are exact in float64 and r = o / u is ONE
    rounding: per decay the float score is s (1 - r~)(1 + d3) with r~ = r (1 + d1), (1 - r~) rounded (1 + d2), |d| <= 2^-53, so its
    relative error grows by at most (r / (1 - r) + 2) 2^-53 plus second-order terms (covered by the factor 1.001); a decay with
    r = 1 gives an exact 0 on both sides.  A pick's bound is the sum over the decays its candidate went through: at most D of them."""
    cand = np.asarray(cand, np.float64).reshape(-1, 5)
    F = lambda v: Fraction(float(v))      # noqa: E731
    box = [[F(v) for v in row[:4]] for row in cand]
    s = [F(np.float32(row[4])) for row in cand]
    err = [Fraction(0)] * len(cand)
    bounds = []
    live = [True] * len(cand)
    ov, thr = F(overlap), F(score_thr)
    slots, scores = [], []
    while any(live) and not (max_out > 0 and len(slots) == max_out):
        m = max((j for j in range(len(cand)) if live[j]), key=lambda j: (s[j], -j))
        if not (s[m] >= thr):
            break
        slots.append(m)
        scores.append(s[m])
        bounds.append(float(err[m] * Fraction(1001, 1000)) * 2.0 ** -53)
        live[m] = False
        A = box[m]
        for j in range(len(cand)):
            if not live[j]:
                continue
            B = box[j]
            iw = min(A[0] + A[2], B[0] + B[2]) - max(A[0], B[0])
            ih = min(A[1] + A[3], B[1] + B[3]) - max(A[1], B[1])
            if iw <= 0 or ih <= 0:
                continue
            o = iw * ih
            r = o / (A[2] * A[3] + B[2] * B[3] - o)
            if r > ov:
                s[j] = s[j] * (1 - r)
                err[j] = err[j] + (r / (1 - r) + 2 if r < 1 else 0)
    return slots, scores, bounds


def hard_order(cand):
    """The slots in plain score order (larger score first, then the lower slot): what the pick order is compared with."""
    cand = np.asarray(cand, np.float64).reshape(-1, 5)
    return np.lexsort((np.arange(len(cand)), -rank_key(cand[:, 4].astype(np.float32).astype(np.float64))))


def soft_facts(cand, dets, slots, decays):
    """What a case must show on the witness's own result before anything is compared with it: (some score was decayed, some
    candidate was dropped, the pick order is not the plain score order of the picked slots)."""
    order = hard_order(cand)
    picked = set(int(v) for v in slots)
    plain = [int(j) for j in order if int(j) in picked]
    return decays > 0, len(slots) < len(np.asarray(cand).reshape(-1, 5)), plain != [int(v) for v in slots]


__all__ = ["soft", "soft_segment", "soft_exact", "soft_facts", "hard_order", "decay_ratio", "candidates_of", "LINEAR", "GAUSSIAN", "METHODS", "mw"]
