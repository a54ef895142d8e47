"""Three witnesses of Seq-NMS over the candidate lists of a clip's frames (mscnn_detections_merge_seq_fwd, Net.set_seq_nms; Han,
Khorrami, Paine et al., "Seq-NMS for Video Object Detection", 2016), on top of merge_witness / vote_witness.candidates_of.  No pin on
the reference -- its scripts run one forward per image and look at no other frame -- so these are the check.

  * seq_nms(): a float64 numpy restatement of the op's contract (include/mscnn_hip.h), steps 1 to 11, for ONE chain: the entered
    boxes of every frame in the merge's order, the links and the in-frame suppression from a numpy spelling of det_overlap<false>,
    the DP with one rounded add per frame, the end box under (larger V, lower t, lower j), score', suppression, the rows of every
    segment.  IEEE operations only: compared bit for bit.
  * seq_exact(): the same loop in exact rationals (fractions.Fraction), overlaps included.  It reports the smallest relative gap
    between a chosen V and its runner-up (a predecessor in step 4, an end box in step 5) and the number of exact ties among them: a
    case with no tie and a gap far above 2^-53 had no pick decided by rounding.
  * brute_best(): for tiny chains, every linked path of live boxes enumerated: the largest exact sum there is.
  * seq_facts(): what a case must show on the witness's own result before anything is compared with it.

TEST INFRASTRUCTURE ONLY."""
from fractions import Fraction

import numpy as np

import merge_witness as mw                       # noqa: F401  (the lists' rows come from its row transforms)
from vote_witness import candidates_of

AVG, MAX = 1, 2
RESCORE = {"avg": AVG, "max": MAX}


def rank_key(s):
    """The score as the merge's order ranks it: a NaN below every number."""
    return np.where(np.isnan(s), -np.inf, s)


def enter(cand, score_thr=0.001, top_k=300):
    """Step 1 for one list: (slots of the boxes that enter, in the merge's order det_key(prob, slot); their scores as doubles)."""
    cand = np.asarray(cand, np.float64).reshape(-1, 5)
    s = cand[:, 4].astype(np.float32).astype(np.float64)      # (double)prob_i: the list holds the prob as a float
    order = np.lexsort((np.arange(len(cand)), -rank_key(s)))
    m = 0
    while m < len(order) and m < top_k and s[order[m]] >= np.float64(score_thr):      # the LEADING ones (a NaN fails)
        m += 1
    return order[:m], s[order[:m]]


def overlap_pairs(A, B):
    """det_overlap<false>(A_i, B_j) for every pair, [a, b] float64, the op's statements one per line; NaN where the op skips the pair
    (iw <= 0, then ih <= 0)."""
    A = np.asarray(A, np.float64).reshape(-1, 4)[:, None, :]
    B = np.asarray(B, np.float64).reshape(-1, 4)[None, :, :]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        iw = np.fmin(A[..., 0] + A[..., 2], B[..., 0] + B[..., 2]) - np.fmax(A[..., 0], B[..., 0])
        ih = np.fmin(A[..., 1] + A[..., 3], B[..., 1] + B[..., 3]) - np.fmax(A[..., 1], B[..., 1])
        o = iw * ih
        u = A[..., 2] * A[..., 3] + B[..., 2] * B[..., 3] - o
        r = o / u
    return np.where((iw <= 0) | (ih <= 0), np.nan, r)


def _entered(cands, score_thr, top_k):
    """Per frame (None: an overflowed list, an empty frame): (slots, scores, boxes) of the boxes that enter."""
    out = []
    for c in cands:
        c = np.zeros((0, 5)) if c is None else np.asarray(c, np.float64).reshape(-1, 5)
        slots, s = enter(c, score_thr, top_k)
        out.append((slots, s, c[slots, :4]))
    return out


def _relations(ent, link_thr, nms_overlap):
    """links[t] [m_t, m_{t-1}] bool (t >= 1) and supp[t] [m_t (the path box), m_t] bool, in float64 as the op computes them."""
    T = len(ent)
    with np.errstate(invalid="ignore"):
        links = [None] + [overlap_pairs(ent[t - 1][2], ent[t][2]).T > np.float64(link_thr) for t in range(1, T)]
        supp = [overlap_pairs(ent[t][2], ent[t][2]) > np.float64(nms_overlap[t]) for t in range(T)]
    return links, supp


def _loop(scores, links, supp, rescore):
    """Steps 3 to 10 in float64.  Returns (score' per frame [m_t] (NaN: never out), seq per frame [m_t] (-1: never out), trace):
    trace = dict(paths = [[(t, j), ...] in frame order] per iteration, dp0 = the path iteration 0's DP held for every box,
    suppressed = [(t, j)], fact6 = some box had >= 2 live linked predecessors and took one that is not the lowest-indexed)."""
    T = len(scores)
    live = [np.ones(len(s), bool) for s in scores]
    oscore = [np.full(len(s), np.nan) for s in scores]
    oq = [np.full(len(s), -1, np.int64) for s in scores]
    total = sum(len(s) for s in scores)
    paths, suppressed, dp0, fact6 = [], [], {}, False
    pairs = [None] + [np.nonzero(links[t]) for t in range(1, T)]
    q = 0
    while any(l.any() for l in live):
        assert q < total, "the loop's bound"
        V, ln, prev = [], [], []
        for t in range(T):                                    # step 4
            s = scores[t]
            m = len(s)
            v, n, p = s.copy(), np.ones(m, np.int64), np.full(m, -1, np.int64)
            if t > 0 and m and len(scores[t - 1]):
                r, c = pairs[t]                               # the linked pairs (j, i), sorted by j then i
                ok = live[t][r] & live[t - 1][c]
                r, c = r[ok], c[ok]
                vals = V[t - 1][c]
                top = np.full(m, -np.inf)
                np.maximum.at(top, r, vals)                   # the largest V among the live linked predecessors of j
                best = np.full(m, len(scores[t - 1]), np.int64)
                eq = vals == top[r]
                np.minimum.at(best, r[eq], c[eq])             # among equal V the lowest i
                first = np.full(m, len(scores[t - 1]), np.int64)
                np.minimum.at(first, r, c)
                has = np.zeros(m, bool)
                has[r] = True
                best = np.where(has, best, 0)
                v = np.where(has, V[t - 1][best] + s, s)      # one rounded add
                n = np.where(has, ln[t - 1][best] + 1, 1)
                p = np.where(has, best, -1)
                fact6 |= bool(np.any((np.bincount(r, minlength=m) >= 2) & has & (best != first)))
            V.append(np.where(live[t], v, -np.inf)); ln.append(n); prev.append(p)
        flat = np.concatenate(V)                              # step 5: (t, j) ascending, the first of equals
        e = int(flat.argmax())
        t = int(np.searchsorted(np.cumsum([len(v) for v in V]), e, side="right"))
        j = e - sum(len(v) for v in V[:t])
        v_end, len_end = V[t][j], int(ln[t][j])

        def back(t, j):
            path = []
            while j >= 0:
                path.append((t, int(j)))
                j = prev[t][j]
                t -= 1
            return path[::-1]

        if q == 0:
            dp0 = {(tt, jj): back(tt, jj) for tt in range(T) for jj in range(len(scores[tt]))}
        path = back(t, j)
        assert len(path) == len_end
        if rescore == AVG:                                    # step 6
            sc = v_end / np.float64(len_end)
        else:
            sc = max(scores[tt][jj] for tt, jj in path)
        for tt, jj in path:                                   # steps 7 and 8
            oscore[tt][jj], oq[tt][jj] = sc, q
            live[tt][jj] = False
            dies = supp[tt][jj] & live[tt]
            suppressed += [(tt, int(k)) for k in np.flatnonzero(dies)]
            live[tt] &= ~dies
        paths.append(path)
        q += 1
    return oscore, oq, dict(paths=paths, dp0=dp0, suppressed=suppressed, fact6=fact6)


def seq_nms(cands, link_thr, nms_overlap, score_thr=0.001, top_k=300, rescore=AVG, max_out=0):
    """One chain: cands = per frame the list [n, 5] float64 [x y w h prob] in slot order (None: the list overflowed, an EMPTY frame);
    nms_overlap: one value per frame.  Returns (per frame (dets [D, 5] = box and score' in output order, slots [D], seq [D]), trace);
    trace also holds ent = per frame (slots, scores, boxes) of the entered boxes, oscore and oq per entered box."""
    ent = _entered(cands, score_thr, top_k)
    links, supp = _relations(ent, link_thr, nms_overlap)
    oscore, oq, trace = _loop([e[1] for e in ent], links, supp, rescore)
    rows = []
    for t, (slots, s, box) in enumerate(ent):
        out = np.flatnonzero(oq[t] >= 0)
        out = out[np.lexsort((out, -oscore[t][out]))]         # step 11: descending score', then the lower sorted position
        if max_out > 0:
            out = out[:max_out]
        rows.append((np.concatenate([box[out], oscore[t][out, None]], 1).reshape(-1, 5), slots[out], oq[t][out]))
    trace.update(ent=ent, oscore=oscore, oq=oq, links=links, supp=supp)
    return rows, trace


def seq_chain(lists, **kw):
    """One chain from its frames' passes (merge_witness.merge's argument per frame; None: overflowed): (per frame (dets, pass [D], row
    [D], candidates, seq [D]), trace)."""
    cands = [None if l is None else candidates_of(l)[0] for l in lists]
    rows, trace = seq_nms(cands, **kw)
    out = []
    for l, (d, slots, seq) in zip(lists, rows):
        if l is None:
            out.append(None)
            continue
        cand, pas = candidates_of(l)
        ids = np.concatenate([np.asarray(i, np.int32) for _, i in l]) if l else np.zeros(0, np.int32)
        out.append((d, pas[slots], ids[slots], len(cand), seq))
    return out, trace


# ---- the same loop in exact rationals ------------------------------------------------------------------------------------------------
def _fr(v):
    return Fraction(float(v))


def _exact_over(A, B, thr):
    """det_overlap<false>(A, B) > thr in rationals (a 0 / 0 is the op's NaN: False)."""
    iw = min(A[0] + A[2], B[0] + B[2]) - max(A[0], B[0])
    if iw <= 0:
        return False
    ih = min(A[1] + A[3], B[1] + B[3]) - max(A[1], B[1])
    if ih <= 0:
        return False
    o = iw * ih
    u = A[2] * A[3] + B[2] * B[3] - o
    return u != 0 and o / u > thr


def seq_exact(cands, link_thr, nms_overlap, score_thr=0.001, top_k=300):
    """Steps 1 to 10 in exact rationals.  Returns dict(paths, sums = the exact V_end per iteration, lives = the live masks before every
    iteration, scores, links (exact), min_gap = the smallest relative gap between a chosen V and its runner-up, ties = how many of
    those choices had an exactly equal runner-up)."""
    ent = _entered(cands, score_thr, top_k)
    T = len(ent)
    S = [[_fr(v) for v in e[1]] for e in ent]
    Bx = [[[_fr(v) for v in b] for b in e[2]] for e in ent]
    lt = _fr(link_thr)
    links = [None] + [[[_exact_over(A, B, lt) for A in Bx[t - 1]] for B in Bx[t]] for t in range(1, T)]
    live = [[True] * len(s) for s in S]
    paths, sums, lives = [], [], []
    gap, ties = None, 0

    def note(best, other):
        nonlocal gap, ties
        if best == other:
            ties += 1
        else:
            g = (best - other) / best
            gap = g if gap is None or g < gap else gap

    while any(any(l) for l in live):
        lives.append([list(l) for l in live])
        V, ln, prev = [], [], []
        for t in range(T):
            v, n, p = [None] * len(S[t]), [0] * len(S[t]), [-1] * len(S[t])
            for j in range(len(S[t])):
                if not live[t][j]:
                    continue
                P = [i for i in range(len(S[t - 1])) if live[t - 1][i] and links[t][j][i]] if t > 0 else []
                if not P:
                    v[j], n[j] = S[t][j], 1
                    continue
                b = P[0]
                for i in P[1:]:
                    if V[t - 1][i] > V[t - 1][b]:
                        b = i
                for i in P:
                    if i != b:
                        note(V[t - 1][b], V[t - 1][i])
                v[j], n[j], p[j] = V[t - 1][b] + S[t][j], ln[t - 1][b] + 1, b
            V.append(v); ln.append(n); prev.append(p)
        end = None
        for t in range(T):
            for j in range(len(S[t])):
                if live[t][j] and (end is None or V[t][j] > V[end[0]][end[1]]):
                    end = (t, j)
        for t in range(T):
            for j in range(len(S[t])):
                if live[t][j] and (t, j) != end:
                    note(V[end[0]][end[1]], V[t][j])
        sums.append(V[end[0]][end[1]])
        path, (t, j) = [], end
        while j >= 0:
            path.append((t, j))
            j = prev[t][j]
            t -= 1
        path = path[::-1]
        for tt, jj in path:
            live[tt][jj] = False
            thr = _fr(nms_overlap[tt])
            for k in range(len(S[tt])):
                if live[tt][k] and _exact_over(Bx[tt][jj], Bx[tt][k], thr):
                    live[tt][k] = False
        paths.append(path)
    return dict(paths=paths, sums=sums, lives=lives, scores=S, links=links, min_gap=float("inf") if gap is None else float(gap), ties=ties)


def brute_best(scores, links, live):
    """The largest sum over EVERY linked path of live boxes (tiny chains: T <= 4, m_t <= 5), by enumeration: a path is any run of live
    boxes of consecutive frames, each linked to the one before.  Every run counts, whether or not it could be extended at either end:
    the maximum over all of them is what steps 4 / 5 must find.  scores / links / live as seq_exact returns them."""
    T = len(scores)
    assert T <= 4 and all(len(s) <= 5 for s in scores), "brute force is for tiny chains"
    best = None

    def walk(t, j, total):
        nonlocal best
        best = total if best is None or total > best else best
        if t + 1 < T:
            for k in range(len(scores[t + 1])):
                if live[t + 1][k] and links[t + 1][k][j]:
                    walk(t + 1, k, total + scores[t + 1][k])

    for t in range(T):
        for j in range(len(scores[t])):
            if live[t][j]:
                walk(t, j, scores[t][j])
    return best


# ---- what a case must show ------------------------------------------------------------------------------------------------------------
def seq_facts(cands, link_thr, nms_overlap, score_thr=0.001, top_k=300):
    """Facts 1 .. 6 on the witness's own result (rescore avg, no max_out):
      1. a path of >= 3 frames exists beside a path of one frame;
      2. some box comes out with score' above its own s (a weak detection rescued), some other with score' below its own;
      3. some box died in step 8 and never came out;
      4. some path does not span all frames: it starts after frame 0 or ends before T - 1;
      5. in some iteration q >= 1 the chosen path differs from what the DP of iteration 0 held for the same end box;
      6. some box had two live linked predecessors and took the one with the larger V, not the lower index."""
    rows, tr = seq_nms(cands, link_thr, nms_overlap, score_thr, top_k, AVG, 0)
    T = len(cands)
    lens = [len(p) for p in tr["paths"]]
    f1 = any(n >= 3 for n in lens) and any(n == 1 for n in lens)
    up = down = False
    for t in range(T):
        s, o = tr["ent"][t][1], tr["oscore"][t]
        out = tr["oq"][t] >= 0
        up |= bool(np.any(o[out] > s[out]))
        down |= bool(np.any(o[out] < s[out]))
    f3 = any(tr["oq"][t][j] < 0 for t, j in tr["suppressed"])
    f4 = any(p[0][0] > 0 or p[-1][0] < T - 1 for p in tr["paths"])
    f5 = any(p != tr["dp0"][p[-1]] for p in tr["paths"][1:])
    return f1, up and down, f3, f4, f5, bool(tr["fact6"])


__all__ = ["seq_nms", "seq_chain", "seq_exact", "brute_best", "seq_facts", "enter", "overlap_pairs", "candidates_of", "AVG", "MAX", "RESCORE"]
