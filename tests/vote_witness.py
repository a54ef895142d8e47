"""Two witnesses of the box vote behind the merge (mscnn_detections_merge_vote_fwd, Net.set_box_voting), on top of merge_witness and
nms_witness.  No pin on the reference -- its scripts neither merge nor vote -- so these are the check.

  * vote(): a numpy restatement in float64.  The voter test in the op's operation order (the NMS's own overlap for ovr_dnm = union:
    iw, skip, ih, skip, o = iw * ih, u = A.w * A.h + B.w * B.h - o, o / u >= thr), the weighted mean in the op's DOCUMENTED summation
    order (include/mscnn_hip.h): 64 partial sums per quantity, partial l over the voters among slots l, l + 64, ... in ascending
    order, each term p * v rounded and then added, the partials combined by an xor butterfly over 32, 16, ..., 1, the result in
    partial 0, then the four divisions.  Compared bit for bit.
  * vote_exact(): the same mean over the voter set vote() found, in exact rational arithmetic (fractions.Fraction), in the manner
    of witness.imresize_exact: what the float witness itself is measured against.

TEST INFRASTRUCTURE ONLY."""
from fractions import Fraction

import numpy as np

import merge_witness as mw

LANES = 64


def candidates_of(passes):
    """The list of one segment in slot order: the passes' rows [n, 5] float64 [x y w h prob] in add order (merge_witness.merge's
    concatenation), and the pass of every slot."""
    rows = np.concatenate([np.asarray(r, np.float64).reshape(-1, 5) for r, _ in passes]) if passes else np.zeros((0, 5))
    pas = np.concatenate([np.full(len(i), k, np.int32) for k, (_, i) in enumerate(passes)]) if passes else np.zeros(0, np.int32)
    return rows, pas


def voter_mask(A, cand, thr):
    """Which candidates vote for the kept box A = [x y w h]: bool [n], the op's statements one per line, all in float64."""
    A = np.asarray(A, np.float64)
    B = np.asarray(cand, np.float64).reshape(-1, 5)
    as_a = A[2] * A[3]
    xe_a = A[0] + A[2]
    ye_a = A[1] + A[3]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        iw = np.fmin(xe_a, B[:, 0] + B[:, 2]) - np.fmax(A[0], B[:, 0])
        ih = np.fmin(ye_a, B[:, 1] + B[:, 3]) - np.fmax(A[1], B[:, 1])
        hit = ~(iw <= 0) & ~(ih <= 0)                # (the op skips a pair on iw <= 0, then on ih <= 0)
        o = iw * ih
        u = as_a + B[:, 2] * B[:, 3] - o
        o = o / u
        return hit & (o >= thr)                      # a NaN ratio does not vote


def weighted_mean(cand, slots):
    """(sum p, [sum p x / sum p, ... y, w, h], voters) over the given slots of the list, in the documented order.  Five float64
    accumulators per partial, +0.0 to begin with."""
    cand = np.asarray(cand, np.float64).reshape(-1, 5)
    acc = np.zeros((5, LANES), np.float64)
    for j in sorted(int(v) for v in slots):          # ascending slot order inside every partial
        l = j % LANES
        p = np.float64(np.float32(cand[j, 4]))       # (double)prob_j: the list holds the prob as a float
        acc[0, l] = acc[0, l] + p
        for q in range(4):
            acc[1 + q, l] = acc[1 + q, l] + p * cand[j, q]
    lanes = np.arange(LANES)
    m = LANES // 2
    while m >= 1:
        acc = acc + acc[:, lanes ^ m]
        m //= 2
    assert all(np.all(acc[q].view(np.uint64) == acc[q, 0].view(np.uint64)) for q in range(5)), "the butterfly leaves one value in every partial"
    with np.errstate(divide="ignore", invalid="ignore"):
        return acc[0, 0], acc[1:, 0] / acc[0, 0], len(slots)


def vote(dets, cand, thr):
    """The kept rows dets [D, 5] of one segment, voted: (rows [D, 5], voter slots per row).  A row with fewer than two voters, or
    whose sum p is not > 0, is returned as it came; prob is never touched."""
    dets = np.array(dets, np.float64).reshape(-1, 5)
    cand = np.asarray(cand, np.float64).reshape(-1, 5)
    out, who = dets.copy(), []
    for k in range(len(dets)):
        slots = np.flatnonzero(voter_mask(dets[k, :4], cand, thr))
        who.append(slots)
        if len(slots) < 2:
            continue
        sp, mean, _ = weighted_mean(cand, slots)
        if sp > 0:
            out[k, :4] = mean
    return out, who


def vote_segment(passes, thr, overlap=0.5, type="maxg", ovr_dnm="union"):
    """One segment from its passes (merge_witness.merge's argument): (un-voted dets, voted dets, pass, row, candidates, voter slots
    per kept row, pass of every slot)."""
    dets, pas, row, n = mw.merge(passes, overlap, type, ovr_dnm)
    cand, cand_pass = candidates_of(passes)
    voted, who = vote(dets, cand, thr)
    return dets, voted, pas, row, n, who, cand_pass


def vote_exact(cand, slots):
    """[x y w h] of the weighted mean over `slots` as exact rationals (every float64 is a rational): sum p v / sum p."""
    cand = np.asarray(cand, np.float64).reshape(-1, 5)
    sp = sum((Fraction(float(np.float32(cand[j, 4]))) for j in slots), Fraction(0))
    return [sum((Fraction(float(np.float32(cand[j, 4]))) * Fraction(float(cand[j, q])) for j in slots), Fraction(0)) / sp for q in range(4)]


def vote_facts(dets, cand, cand_pass, who):
    """What a case must show on the witness's own result before anything is compared with it: some kept row has (voters from more
    than one pass, a voter with a higher score than its own -- a candidate another kept box suppressed --, fewer than two voters)."""
    multi = higher = lonely = False
    for k, slots in enumerate(who):
        multi |= len(set(np.asarray(cand_pass)[slots].tolist())) > 1
        higher |= bool(np.any(np.asarray(cand)[slots, 4] > dets[k, 4]))
        lonely |= len(slots) < 2
    return multi, higher, lonely
