"""The witness of mscnn_tracks_update_assign_fwd (include/mscnn_hip.h): steps 4'' and 5'', the optimal assignment, in Python integers.

match_optimal has the signature every witness's `match=` takes, so track_witness.update, track_kalman_witness.update and
track_streams_witness.run run it unchanged.  It is the header's statement, line for line: integer weights, shortest augmenting paths
with potentials, a private dummy column per row.  update / run / run_streams step a table and add the passes' search steps to the
slot's "steps" (header word 5, MSCNN_TRACKS_STEPS), saturating at INT32_MAX; state_bytes / parse_state speak that word.

A plain helper module: `import track_assign_witness as aw`.
"""
import math

import numpy as np

import track_kalman_witness as kw
import track_streams_witness as sw
import track_witness as tw

GREEDY, OPTIMAL = 1, 2                   # MSCNN_TRACK_ASSIGN_*
STEPS_WORD = 5                           # MSCNN_TRACKS_STEPS
INT32_MAX = 2 ** 31 - 1
INF = None                               # minv of a column no step has reached


def q(x):
    """floor(x * 2^30) as an integer: exact in double (a scaling by a power of two, then floor)."""
    return int(math.floor(float(x) * 1073741824.0))


def weights(r, thr, tracks, dets):
    """{(i, j): w} of the eligible pairs (r > thr; a NaN is no pair): w = q(r) - q(thr) + 1 >= 1."""
    tracks, dets = list(tracks), list(dets)
    if not tracks or not dets:
        return {}
    qt = q(thr)
    sub = np.asarray(r)[np.ix_(tracks, dets)]
    with np.errstate(invalid="ignore"):
        ii, jj = np.nonzero(sub > thr)
    return {(tracks[a], dets[b]): q(sub[a, b]) - qt + 1 for a, b in zip(ii.tolist(), jj.tolist())}


def match_optimal(r, thr, tracks, dets):
    """The maximum-weight matching over the eligible pairs of `tracks` x `dets` (index lists, ascending).  Returns ({i: j}, steps)."""
    tracks, dets = list(tracks), list(dets)
    with np.errstate(invalid="ignore"):
        w = weights(r, thr, tracks, dets)
    a, b = len(tracks), len(dets)
    # columns: 0 .. b - 1 the detections in ascending j, b + x the private dummy of row x; -1 the virtual start
    cost = [dict() for _ in range(a)]
    row_of, col_of = {i: x for x, i in enumerate(tracks)}, {j: c for c, j in enumerate(dets)}
    for (i, j), v in w.items():
        cost[row_of[i]][col_of[j]] = -v
    for x in range(a):
        cost[x][b + x] = 0
    u = [0] * a
    v = [0] * (b + a)
    p = [None] * (b + a)      # the row of a column; None: free
    steps = 0
    bound = min(a, b) + 1
    for x in range(a):
        if len(cost[x]) == 1:      # no eligible pair: unmatched, no step
            continue
        minv = [INF] * (b + a)
        way = [None] * (b + a)
        used = [False] * (b + a)
        seen = []      # the columns with a finite minv, the used ones among them: the loops below need no others
        i0, j0 = x, -1
        for _ in range(bound):
            steps += 1
            for c, cc in cost[i0].items():
                if used[c]:
                    continue
                cur = cc - u[i0] - v[c]
                if minv[c] is INF:
                    seen.append(c)
                if minv[c] is INF or cur < minv[c]:
                    minv[c] = cur
                    way[c] = j0
            # the lowest column among equals, real columns before dummies
            delta, j1 = min((minv[c], c) for c in seen if not used[c])
            u[x] += delta
            for c in seen:
                if used[c]:
                    u[p[c]] += delta
                    v[c] -= delta
                else:
                    minv[c] -= delta
            used[j1] = True
            j0 = j1
            if p[j1] is None:
                break
            i0 = p[j1]
        else:
            raise AssertionError("a search took more than min(a, b) + 1 steps")
        while j0 != -1:      # augment back along way
            jp = way[j0]
            p[j0] = x if jp == -1 else p[jp]
            j0 = jp
    return {tracks[p[c]]: dets[c] for c in range(b) if p[c] is not None}, steps


def total_weight(r, thr, pairs):
    qt = q(thr)
    return sum(q(r[i, j]) - qt + 1 for i, j in pairs.items())


def brute_force(r, thr, tracks, dets):
    """The largest total weight of any matching over the eligible pairs, by exhaustive search (small cases only)."""
    with np.errstate(invalid="ignore"):
        w = weights(r, thr, tracks, dets)
    tracks, dets = list(tracks), list(dets)

    def rest(at, taken):      # every row: unmatched, or any free detection it is eligible with
        if at == len(tracks):
            return 0
        best = rest(at + 1, taken)
        for j in dets:
            if j not in taken and (tracks[at], j) in w:
                best = max(best, w[(tracks[at], j)] + rest(at + 1, taken | {j}))
        return best
    return rest(0, frozenset())


def cluster(rng, a, b, sigma=6.0, points=3, lo=20.0, hi=30.0):
    """The issue's generator: a + b boxes, centres jittered with sigma around `points` points, sizes lo .. hi.  Returns (A, B) [., 4]."""
    cen = rng.uniform(40.0, 200.0, size=(points, 2))

    def boxes(n):
        c = cen[rng.integers(0, points, size=n)] + rng.normal(0.0, sigma, size=(n, 2))
        s = rng.uniform(lo, hi, size=(n, 2))
        return np.concatenate([c - s / 2, s], axis=1)
    return boxes(a), boxes(b)


def dense(rng, n, sigma=2.0, size=40.0):
    """A dense n x n cluster: centres sigma around one point, one size."""
    def boxes():
        c = np.array([100.0, 100.0]) + rng.normal(0.0, sigma, size=(n, 2))
        return np.concatenate([c - size / 2, np.full((n, 2), size)], axis=1)
    return boxes(), boxes()


# ---- a table under the optimal form: the witnesses' update with match_optimal, the steps summed into the slot
class Counting:
    """match_optimal that sums the steps of the passes it ran."""

    def __init__(self):
        self.steps = 0
        self.most = 0      # the most steps of one pass

    def __call__(self, r, thr, tracks, dets):
        pairs, k = match_optimal(r, thr, tracks, dets)
        self.steps += k
        self.most = max(self.most, k)
        return pairs, k


def add_steps(slot, k):
    slot["steps"] = min(slot.get("steps", 0) + k, INT32_MAX)


def update(slot, rows, p, max_tracks, kp=None, assign=OPTIMAL):
    """One frame of one slot in place; kp (track_kalman_witness.kparams): the Kalman form.  Returns the frame's ids."""
    m = Counting() if assign == OPTIMAL else tw.match_walk
    ids = tw.update(slot, rows, p, max_tracks, m) if kp is None else kw.update(slot, rows, p, kp, max_tracks, m)
    add_steps(slot, m.steps if assign == OPTIMAL else 0)
    return ids


def run(slots, frames, p, max_tracks, kp=None, assign=OPTIMAL):
    """frames[t][k]; returns ids[t][k]."""
    return [[update(slots[k], fr[k], p, max_tracks, kp, assign) for k in range(len(slots))] for fr in frames]


def run_streams(tables, frames, stream_of, p, max_tracks, kp=None, assign=OPTIMAL):
    """tables[s][k] stepped through the frames of stream s (in place); ids[t][k] in call order."""
    ids = [None] * len(frames)
    for s, tab in enumerate(tables):
        for t in [t for t, o in enumerate(stream_of) if o == s]:
            ids[t] = [update(tab[k], frames[t][k], p, max_tracks, kp, assign) for k in range(len(tab))]
    return ids


def state_bytes(slots, max_tracks, base, assign=OPTIMAL):
    """track_witness.state_bytes, then word 5 of every header: the slot's steps under OPTIMAL, 0 under GREEDY."""
    out = tw.state_bytes(slots, max_tracks, base)
    slot_b = tw.state_layout(len(slots), max_tracks)[2]
    for k, s in enumerate(slots):
        out[k * slot_b:k * slot_b + 32].view(np.int32)[STEPS_WORD] = s.get("steps", 0) if assign == OPTIMAL else 0
    return out


def parse_state(buf, K, max_tracks):
    """track_witness.parse_state plus "steps" from word 5."""
    slots = tw.parse_state(buf, K, max_tracks)
    slot_b = tw.state_layout(K, max_tracks)[2]
    buf = np.asarray(buf, np.uint8)
    for k, s in enumerate(slots):
        s["steps"] = int(buf[k * slot_b:k * slot_b + 32].view(np.int32)[STEPS_WORD])
    return slots


def steps_of(buf, K, max_tracks):
    """Word 5 of every table of a state buffer."""
    return [s["steps"] for s in parse_state(buf, K, max_tracks)]


__all__ = ["match_optimal", "update", "run", "run_streams", "state_bytes", "parse_state", "sw"]
