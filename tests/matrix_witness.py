"""Witnesses of Matrix NMS over the merged candidates (mscnn_detections_merge_matrix_fwd, Net.set_matrix_nms; Wang et al., SOLOv2,
NeurIPS 2020, Algorithm 1), on top of merge_witness, vote_witness.candidates_of and soft_witness.decay_ratio.  No pin on the
reference -- its scripts neither merge nor decay a score -- so these are the check.

  * matrix(): a float64 numpy restatement of the seven steps of the op's contract (include/mscnn_hip.h), statement for statement:
    the merge's order, the union overlap with non-hits set to 0.0, the column maximum as compensation, the decay as an np.fmin /
    np.fmax reduction over the higher-ranked candidates, one exp per candidate, the output in descending score' order.  The LINEAR
    method is compared bit for bit (IEEE operations only, and min / max of doubles are exact in any order); the GAUSSIAN one calls
    exp once per candidate, numpy's here and OCML's on the device.
  * matrix_naive(): the same contract as a plain triple loop over Python floats; it shares no vectorised line with matrix().
  * matrix_exact(): the linear method in exact rationals (fractions.Fraction), with the relative error bound of the float result.
  * matrix_facts(): what a case must show on the witness's own result before anything is compared with it.

TEST INFRASTRUCTURE ONLY."""
import math
from fractions import Fraction

import numpy as np

import merge_witness as mw
import soft_witness as sw
from vote_witness import candidates_of

LINEAR, GAUSSIAN = 1, 2
METHODS = {"linear": LINEAR, "gaussian": GAUSSIAN}


def sorted_order(cand):
    """Step 1: the slots in the merge's own order -- larger prob first, then the earlier slot (det_key(prob, slot))."""
    cand = np.asarray(cand, np.float64).reshape(-1, 5)
    s = cand[:, 4].astype(np.float32).astype(np.float64)
    return np.lexsort((np.arange(len(cand)), -s))


def ratios_below(c, i):
    """Step 2: r_ij of sorted box i against every j > i -- soft_witness.decay_ratio's overlap lines, non-hits set to 0.0."""
    hit, r = sw.decay_ratio(c[i, :4], c[i + 1:])
    return np.where(hit, r, 0.0)


def matrix(cand, method, sigma=0.5, score_thr=0.001, max_out=0):
    """One segment: cand [n, 5] float64 [x y w h prob] in slot order.  Returns (dets [D, 5] with score', slots [D] in output order,
    info): info["order"] the slots in sorted order, info["scores"] score' per sorted position, info["comp"] c per sorted position,
    info["decayed"] how many scores changed, info["comp_mattered"] for how many j the minimising term has c_i > 0 and exceeds
    1 - r_ij (linear only), info["min_gap"] the smallest relative gap between adjacent output scores and between any score and
    score_thr."""
    cand = np.asarray(cand, np.float64).reshape(-1, 5)
    n = len(cand)
    order = sorted_order(cand)
    c = cand[order]
    s = c[:, 4].astype(np.float32).astype(np.float64)      # (double)prob_j: the list holds the prob as a float
    sigma, score_thr = np.float64(sigma), np.float64(score_thr)
    comp = np.zeros(n, np.float64)                          # step 3: c_0 = 0.0, the maximum starts from 0.0
    for i in range(n - 1):
        comp[i + 1:] = np.fmax(comp[i + 1:], ratios_below(c, i))
    mattered = np.zeros(n, bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if method == LINEAR:                                # step 4
            d = np.ones(n, np.float64)
            for i in range(n - 1):
                den = 1.0 - comp[i]
                if not den > 0:
                    continue
                r = ratios_below(c, i)
                term = (1.0 - r) / den
                lower = term < d[i + 1:]
                mattered[i + 1:] = np.where(lower, (comp[i] > 0) & (term > 1.0 - r), mattered[i + 1:])
                d[i + 1:] = np.fmin(d[i + 1:], term)
            score = s * d
        else:                                               # step 5
            g = np.zeros(n, np.float64)
            for i in range(n - 1):
                r = ratios_below(c, i)
                g[i + 1:] = np.fmax(g[i + 1:], (r * r - comp[i] * comp[i]) / sigma)
            score = s * np.exp(-g)
        if n:
            score[0] = s[0]                                 # step 6
        kept = np.flatnonzero(score >= score_thr)           # step 7 (a NaN fails the test)
        out = kept[np.argsort(-score[kept], kind="stable")]
        if max_out > 0:
            out = out[:max_out]
        gaps = [np.inf]
        if n:
            gaps.append(np.nanmin(np.abs(score - score_thr) / np.abs(score)))
        full = kept[np.argsort(-score[kept], kind="stable")]
        if len(full) > 1:
            gaps.append(np.min((score[full][:-1] - score[full][1:]) / np.abs(score[full][:-1])))
        decayed = int(np.count_nonzero(score != s))
    dets = np.concatenate([c[out, :4], score[out, None]], 1) if len(out) else np.zeros((0, 5))
    info = dict(order=order, scores=score, comp=comp, decayed=decayed, comp_mattered=int(np.count_nonzero(mattered)),
                min_gap=float(np.min(gaps)))
    return dets.reshape(-1, 5), order[out].astype(np.int64), info


def matrix_segment(passes, method, sigma=0.5, score_thr=0.001, max_out=0):
    """One segment from its passes (merge_witness.merge's argument): (dets, pass [D], row [D], candidates, slots, info, cand)."""
    cand, cand_pass = candidates_of(passes)
    ids = np.concatenate([np.asarray(i, np.int32) for _, i in passes]) if passes else np.zeros(0, np.int32)
    dets, slots, info = matrix(cand, method, sigma, score_thr, max_out)
    return dets, cand_pass[slots], ids[slots], len(cand), slots, info, cand


def matrix_naive(cand, method, sigma=0.5, score_thr=0.001, max_out=0):
    """The contract as a plain triple loop over Python floats (IEEE doubles): (dets, slots)."""
    rows = [[float(v) for v in row] for row in np.asarray(cand, np.float64).reshape(-1, 5)]
    n = len(rows)
    prob = [float(np.float32(row[4])) for row in rows]
    order = sorted(range(n), key=lambda k: (-prob[k], k))
    box = [rows[k][:4] for k in order]
    s = [prob[k] for k in order]
    nan = float("nan")

    def fmin(a, b):
        return b if a != a else (a if b != b else (b if b < a else a))

    def fmax(a, b):
        return b if a != a else (a if b != b else (b if b > a else a))

    def div(a, b):
        try:
            return a / b
        except ZeroDivisionError:
            return nan if a == 0 or a != a else math.copysign(math.inf, a) * math.copysign(1.0, b)

    def ratio(A, B):
        iw = fmin(A[0] + A[2], B[0] + B[2]) - fmax(A[0], B[0])
        if iw <= 0:
            return 0.0
        ih = fmin(A[1] + A[3], B[1] + B[3]) - fmax(A[1], B[1])
        if ih <= 0:
            return 0.0
        o = iw * ih
        u = A[2] * A[3] + B[2] * B[3] - o
        r = div(o, u)
        return 0.0 if r != r else r

    rr = [[ratio(box[i], box[j]) for j in range(i + 1, n)] for i in range(n)]      # rr[i][j - i - 1] = r_ij, each pair once
    score = []
    comp = []
    for j in range(n):
        cj = 0.0
        for k in range(j):
            cj = fmax(cj, rr[k][j - k - 1])
        comp.append(cj)
    for j in range(n):
        if method == LINEAR:
            d = 1.0
            for i in range(j):
                den = 1.0 - comp[i]
                if den > 0:
                    d = fmin(d, div(1.0 - rr[i][j - i - 1], den))
            score.append(s[j] * d if j else s[j])
        else:
            g = 0.0
            for i in range(j):
                r = rr[i][j - i - 1]
                g = fmax(g, div(r * r - comp[i] * comp[i], float(sigma)))
            score.append(s[j] * math.exp(-g) if j else s[j])
    out = []
    for j in range(n):                                      # the output position of j: how many kept candidates precede it
        if not score[j] >= score_thr:
            continue
        before = 0
        for k in range(n):
            if score[k] >= score_thr and (score[k] > score[j] or (score[k] == score[j] and k < j)):
                before += 1
        out.append((before, j))
    out = [j for _, j in sorted(out)]
    if max_out > 0:
        out = out[:max_out]
    dets = np.array([box[j] + [score[j]] for j in out], np.float64).reshape(-1, 5)
    return dets, np.array([order[j] for j in out], np.int64)


def matrix_exact(cand):
    """The linear method in exact rationals (every float64 is one): (order: the slots in sorted order, the exact score' of every
    sorted position, the relative error bound of the float64 score' of every sorted position).

    The bound, for boxes whose coordinates are small integers -- then iw, ih, o and u are exact in float64, so r~ = r (1 + d1) is
    ONE rounding, and c~_i, a maximum of such roundings, is the rounding of the exact maximum (rounding is monotone): c~ = c (1 + d2).
    With u = 2^-53 and every |d| <= u, a term of the minimum is computed as
        fl(1 - r~) = (1 - r) (1 - r d1 / (1 - r)) (1 + d3)        relative error <= (r / (1 - r) + 1) u
        fl(1 - c~) = (1 - c) (1 - c d2 / (1 - c)) (1 + d4)        relative error <= (c / (1 - c) + 1) u
        the division                                              one more rounding
    so t~ = t (1 + e) with |e| <= (r / (1 - r) + c / (1 - c) + 3) u to first order.  A term with r = 1 is an exact 0 on both sides;
    a term with 1 - c = 0 is skipped on both sides (c~ = 1 exactly when c = 1: o / u of small integers is either 1 or at least 1 / u
    away from it); a term with r = 0 is 1 / (1 - c) >= 1 on both sides and never lowers the minimum, which starts from 1.0.  The
    minimum of perturbed terms lies within the largest perturbation of any term that can lower it: with i* the exact minimiser and
    k the float one, d~ <= t~_i* <= d (1 + e_i*) and d~ = t~_k >= t_k (1 - e_k) >= d (1 - e_k).  E_j = the largest e over the
    overlapping i < j therefore bounds the decay, the product s_j * d~_j adds one rounding, and the factor 1.001 covers the
    second-order terms: bound_j = 1.001 (E_j + 1) u, and 0 where no term lowered the start (score'_j = s_j exactly)."""
    cand = np.asarray(cand, np.float64).reshape(-1, 5)
    order = sorted_order(cand)
    F = lambda v: Fraction(float(v))      # noqa: E731
    c = cand[order]
    box = [[F(v) for v in row[:4]] for row in c]
    s = [F(np.float32(row[4])) for row in c]
    n = len(c)
    xe, ye = c[:, 0] + c[:, 2], c[:, 1] + c[:, 3]
    pairs = {}
    for i in range(n):                                      # (the overlapping pairs, found in floats: the comparisons are exact)
        hit = np.flatnonzero((np.minimum(xe[i], xe[i + 1:]) - np.maximum(c[i, 0], c[i + 1:, 0]) > 0) &
                             (np.minimum(ye[i], ye[i + 1:]) - np.maximum(c[i, 1], c[i + 1:, 1]) > 0)) + i + 1
        for j in hit:
            A, B = box[i], box[int(j)]
            iw = min(A[0] + A[2], B[0] + B[2]) - max(A[0], B[0])
            ih = min(A[1] + A[3], B[1] + B[3]) - max(A[1], B[1])
            o = iw * ih
            pairs[(i, int(j))] = o / (A[2] * A[3] + B[2] * B[3] - o)
    comp = [Fraction(0)] * n
    for (i, j), r in pairs.items():
        comp[j] = max(comp[j], r)
    d = [Fraction(1)] * n
    E = [Fraction(-1)] * n
    for (i, j), r in pairs.items():
        if comp[i] >= 1:
            continue
        d[j] = min(d[j], (1 - r) / (1 - comp[i]))
        if r < 1:
            E[j] = max(E[j], r / (1 - r) + comp[i] / (1 - comp[i]) + 3)
        else:
            E[j] = max(E[j], Fraction(0))
    scores = [s[j] * d[j] for j in range(n)]
    bounds = [0.0 if E[j] < 0 else float((E[j] + 1) * Fraction(1001, 1000)) * 2.0 ** -53 for j in range(n)]
    return order, scores, bounds


def matrix_facts(cand, dets, slots, info, score_thr, soft_overlap=0.5):
    """(a) some score was decayed, (b) some candidate fell below score_thr, (c) the output order is not the input's sorted order,
    (d) for some j the minimising term has c_i > 0 and exceeds 1 - r_ij: the compensation mattered, (e) the scores differ from
    soft_witness.soft(..., LINEAR) on the same list: the op is not Soft-NMS under another name."""
    cand = np.asarray(cand, np.float64).reshape(-1, 5)
    plain = [int(k) for k in info["order"] if int(k) in set(int(v) for v in slots)]
    sd = sw.soft(cand, sw.LINEAR, overlap=soft_overlap, score_thr=score_thr, max_out=200)[0]      # (its first 200 picks say enough)
    differs = len(sd) != min(len(dets), 200) or not np.array_equal(sd[:, 4], dets[:len(sd), 4])
    return (info["decayed"] > 0, len(slots) < len(cand), plain != [int(v) for v in slots], info["comp_mattered"] > 0, bool(differs))


__all__ = ["matrix", "matrix_segment", "matrix_naive", "matrix_exact", "matrix_facts", "sorted_order", "candidates_of", "LINEAR",
           "GAUSSIAN", "METHODS", "mw", "sw"]
