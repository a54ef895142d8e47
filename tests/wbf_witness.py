"""Two witnesses of weighted boxes fusion over the merged candidates (mscnn_detections_merge_wbf_fwd, Net.set_wbf; Solovyev, Wang,
Gabruseva, 2019 / 2021), on top of merge_witness and vote_witness.candidates_of.  No pin on the reference -- its scripts run one
forward per image and neither merge nor fuse -- so these are the check.

  * wbf(): a float64 numpy restatement of the op's contract (include/mscnn_hip.h), statement for statement: walk the candidates in
    the merge's order while s >= skip_thr && s > 0, match each against the fused boxes of the clusters that exist (the vote's overlap
    statements with A = the fused box, the largest r > thr, among equal r the lowest cluster), open a cluster or add the candidate
    to the running sums -- the product rounded, then the sum, in walk order -- and divide; conf per cluster, the clusters in
    descending conf.  IEEE operations only: compared bit for bit.  It also returns min_gap: the smallest relative gap the walk saw
    between a best r and thr, a best r and the runner-up above thr, or two neighbouring conf of the output order -- how far the
    inputs are from a decision that a last-bit difference could turn.
  * wbf_exact(): the same walk in exact rational arithmetic (fractions.Fraction), with a derived bound on the float walk's fused
    coordinates: what the float witness itself is measured against.

TEST INFRASTRUCTURE ONLY."""
from fractions import Fraction

import numpy as np

import merge_witness as mw
from vote_witness import candidates_of

AVG, MAX = 1, 2
CONF_TYPES = {"avg": AVG, "max": MAX}


def rank_key(s):
    """The score as the merge's order ranks it: a NaN below every number."""
    return np.where(np.isnan(s), -np.inf, s)


def walk_order(cand):
    """The slots in the merge's own order, det_key(prob, slot): larger prob first, then the lower slot."""
    cand = np.asarray(cand, np.float64).reshape(-1, 5)
    return np.lexsort((np.arange(len(cand)), -rank_key(cand[:, 4].astype(np.float32).astype(np.float64))))


def match_ratio(F, B):
    """(hit, r) of the fused boxes F [C, 4] (A of the contract) against the walked box B = [x y w h]: the op's statements one per
    line, all in float64.  hit: the op reached the ratio (it skips a pair on iw <= 0, then on ih <= 0) and the ratio is no NaN."""
    F = np.asarray(F, np.float64).reshape(-1, 4)
    B = np.asarray(B, np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        iw = np.fmin(F[:, 0] + F[:, 2], B[0] + B[2]) - np.fmax(F[:, 0], B[0])
        ih = np.fmin(F[:, 1] + F[:, 3], B[1] + B[3]) - np.fmax(F[:, 1], B[1])
        o = iw * ih
        u = F[:, 2] * F[:, 3] + B[2] * B[3] - o
        r = o / u
    return ~(iw <= 0) & ~(ih <= 0) & ~np.isnan(r), r


def _rel(a, b):
    """|a - b| / |a| as a float, 0.0 for a NaN or a 0 / 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.abs(np.float64(a) - np.float64(b)) / np.abs(np.float64(a))
    return 0.0 if np.isnan(g) else float(g)


def _walk(cand, thr, skip_thr):
    """Steps 1 to 5.  Returns a dict: C, F [C, 4], sums [C, 5] (sw sx sy sW sH), members [C], first [C] (slots), s (the scores as
    doubles), cluster_of [n] (-1: never entered), min_gap of the matches, and per entered candidate a record
    (slot, joined cluster or -1, clusters above thr, whether it overlaps the joined cluster's FIRST member's box by more than thr)."""
    cand = np.asarray(cand, np.float64).reshape(-1, 5)
    n = len(cand)
    s = cand[:, 4].astype(np.float32).astype(np.float64)      # (double)prob_i: the list holds the prob as a float
    thr, skip_thr = np.float64(thr), np.float64(skip_thr)
    F, sums = np.zeros((n, 4)), np.zeros((n, 5))
    members, first = np.zeros(n, np.int64), np.zeros(n, np.int64)
    cluster_of = np.full(n, -1, np.int64)
    C, min_gap, records = 0, np.inf, []
    for i in walk_order(cand):
        si, B = s[i], cand[i, :4]
        if not (si >= skip_thr and si > 0):
            break                                             # the order makes this the same as filtering
        hit, r = match_ratio(F[:C], B)
        above = np.flatnonzero(hit & (r > thr))
        rr = np.where(hit, r, -np.inf)
        if C:
            best = float(rr.max())
            if best > -np.inf:
                min_gap = min(min_gap, _rel(thr, best))
        if len(above) == 0:
            c = C
            sums[c] = [si, si * B[0], si * B[1], si * B[2], si * B[3]]
            members[c], first[c] = 1, i
            F[c] = B                                          # bit for bit
            C += 1
            records.append((int(i), -1, above, True))
        else:
            c = int(above[np.argmax(r[above])])               # (argmax: the first of equals, the lowest cluster)
            if len(above) > 1:
                top = np.sort(r[above])
                min_gap = min(min_gap, _rel(top[-1], top[-2]))
            sums[c, 0] = sums[c, 0] + si
            for q in range(4):
                sums[c, 1 + q] = sums[c, 1 + q] + si * B[q]   # the product rounded, then the sum
            members[c] += 1
            h1, r1 = match_ratio(cand[first[c], :4][None], B)
            records.append((int(i), c, above, bool(h1[0] and r1[0] > thr)))
            with np.errstate(divide="ignore", invalid="ignore"):
                F[c] = sums[c, 1:] / sums[c, 0]
        cluster_of[i] = c
    return dict(C=C, F=F[:C], sums=sums[:C], members=members[:C], first=first[:C], s=s, cluster_of=cluster_of, min_gap=min_gap, records=records)


def _finish(w, conf_type, expected, max_out):
    """Steps 6 and 7 on a walk: (dets [D, 5], first slots [D], members [D], the output order's cluster indices (all C), min conf gap)."""
    C, T = w["C"], int(expected)
    m = w["members"]
    with np.errstate(divide="ignore", invalid="ignore"):
        conf = w["sums"][:, 0] / m.astype(np.float64) if conf_type == AVG else w["s"][w["first"]]
        conf = conf * np.minimum(m, T).astype(np.float64) / np.float64(T)
    order = np.lexsort((np.arange(C), -conf))                # descending conf, then the lower cluster
    gap = np.inf
    for a, b in zip(order[:-1], order[1:]):
        gap = min(gap, _rel(conf[a], conf[b]))
    out = order[:max_out] if max_out > 0 else order
    dets = np.concatenate([w["F"][out], conf[out, None]], 1).reshape(-1, 5)
    return dets, w["first"][out], m[out], order, gap


def wbf(cand, thr=0.55, skip_thr=0.0, conf_type=AVG, expected=1, max_out=0):
    """One segment: cand [n, 5] float64 [x y w h prob] in slot order.  Returns (dets [D, 5] = fused box and conf in output order,
    first-member slots [D], members [D], the cluster (creation index) of every candidate [n], -1 for one that never entered, min_gap)."""
    w = _walk(cand, thr, skip_thr)
    dets, first, members, order, gap = _finish(w, conf_type, expected, max_out)
    return dets, first, members, w["cluster_of"], min(w["min_gap"], gap)


def wbf_segment(passes, thr=0.55, skip_thr=0.0, conf_type=AVG, expected=1, max_out=0):
    """One segment from its passes (merge_witness.merge's argument): (dets, pass [D], row [D], candidates, first slots, members,
    cluster_of, min_gap)."""
    cand, cand_pass = candidates_of(passes)
    ids = np.concatenate([np.asarray(i, np.int32) for _, i in passes]) if passes else np.zeros(0, np.int32)
    dets, first, members, cluster_of, min_gap = wbf(cand, thr, skip_thr, conf_type, expected, max_out)
    return dets, cand_pass[first], ids[first], len(cand), first, members, cluster_of, min_gap


def wbf_exact(cand, thr=0.55, skip_thr=0.0):
    """The walk (steps 1 to 5) in exact rationals (every float64 is one): (the cluster of every candidate, -1 for one that never
    entered; the exact fused box of every cluster as four Fractions; members per cluster; the relative error bound of the float64
    fused coordinates per cluster).
    The bound, for boxes with x, y, w, h >= 0 and scores > 0 (every term of every sum is then non-negative, so the relative error of
    a sum is at most the largest relative error among its terms' accumulated factors): a cluster of k members has, per coordinate,
    the float numerator  sum_j s_j v_j (1 + d_j) prod (1 + e)  -- one rounding d_j of the product, then at most k - 1 roundings e of
    the additions that follow it in walk order: relative error <= k 2^-53 to first order --, the float denominator sw the same
    without the products: <= (k - 1) 2^-53; the division adds one rounding.  Sum: 2 k 2^-53, second-order terms covered by the
    factor 1.001.  A cluster of one is its candidate's box bit for bit: bound 0."""
    cand = np.asarray(cand, np.float64).reshape(-1, 5)
    n = len(cand)
    Fr = lambda v: Fraction(float(v))      # noqa: E731
    box = [[Fr(v) for v in row[:4]] for row in cand]
    s = [Fr(np.float32(row[4])) for row in cand]
    t, sk = Fr(thr), Fr(skip_thr)
    fused, sums, members = [], [], []
    cluster_of = [-1] * n
    for i in (int(v) for v in walk_order(cand)):
        if not (s[i] >= sk and s[i] > 0):
            break
        B = box[i]
        best, bc = None, -1
        for c, A in enumerate(fused):
            iw = min(A[0] + A[2], B[0] + B[2]) - max(A[0], B[0])
            ih = min(A[1] + A[3], B[1] + B[3]) - max(A[1], B[1])
            if iw <= 0 or ih <= 0:
                continue
            o = iw * ih
            u = A[2] * A[3] + B[2] * B[3] - o
            if u == 0:
                continue
            r = o / u
            if r > t and (best is None or r > best):
                best, bc = r, c
        if bc < 0:
            bc = len(fused)
            fused.append(list(B)); sums.append([s[i]] + [s[i] * v for v in B]); members.append(1)
        else:
            sums[bc][0] += s[i]
            for q in range(4):
                sums[bc][1 + q] += s[i] * B[q]
            members[bc] += 1
            fused[bc] = [sums[bc][1 + q] / sums[bc][0] for q in range(4)]
        cluster_of[i] = bc
    bounds = [0.0 if k == 1 else 2 * k * 1.001 * 2.0 ** -53 for k in members]
    return np.array(cluster_of, np.int64), fused, np.array(members, np.int64), bounds


def wbf_facts(cand, thr=0.55, skip_thr=0.0, conf_type=AVG, expected=1):
    """What a case must show on the witness's own result before anything is compared with it:
      1. some cluster has >= 2 members, and some cluster has exactly 1;
      2. some candidate joined a cluster whose FIRST member's box it does not overlap by more than thr: the fused box moved -- what
         tells WBF from NMS + vote;
      3. some candidate had >= 2 clusters above thr and joined one that is not the lowest-indexed of them: the argmax matters;
      4. the output order is not the creation order: the members / T scaling (or the mean) re-ranked;
      5. some candidate failed skip_thr."""
    cand = np.asarray(cand, np.float64).reshape(-1, 5)
    w = _walk(cand, thr, skip_thr)
    order = _finish(w, conf_type, expected, 0)[3]
    m = w["members"]
    f1 = bool(np.any(m >= 2) and np.any(m == 1))
    f2 = any(c >= 0 and not near_first for _, c, _, near_first in w["records"])
    f3 = any(c >= 0 and len(above) >= 2 and c != int(above.min()) for _, c, above, _ in w["records"])
    f4 = bool(np.any(order != np.arange(len(order))))
    f5 = len(w["records"]) < len(cand)
    return f1, f2, f3, f4, f5


__all__ = ["wbf", "wbf_segment", "wbf_exact", "wbf_facts", "walk_order", "match_ratio", "candidates_of", "AVG", "MAX", "CONF_TYPES", "mw"]
