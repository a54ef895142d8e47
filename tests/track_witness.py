"""The witness of mscnn_tracks_update_fwd (include/mscnn_hip.h): the ten steps in float64 numpy, bit for bit.

A plain helper module: `from tests import track_witness as tw`.  The walk of step 4 is done literally (sort every eligible pair, walk
the sorted list) by match_walk and as rounds of "match every mutually-best pair" by match_rounds, the form the kernel runs; update()
takes either.  pack_bytes / state_bytes / parse_state speak the op's buffers, so the GPU tests compare bytes.
"""
import numpy as np

NONE, LINEAR = 1, 2                      # MSCNN_TRACK_MOTION_*
MOTIONS = {"none": NONE, "linear": LINEAR}
MAX_DETS = 1024                          # detections of a frame that enter
HEADER_WORDS, RECORD_BYTES = 8, 104      # mscnn_tracks_state_layout_of
RECORD = np.dtype([("box", "<f8", 4), ("obs", "<f8", 4), ("vel", "<f8", 2), ("score", "<f8"), ("id", "<i4"), ("hits", "<i4"),
                   ("misses", "<i4"), ("confirmed", "<i4")])
assert RECORD.itemsize == RECORD_BYTES


def params(high_thr=0.5, low_thr=0.1, new_thr=None, match_thr=0.3, match_thr_low=0.5, motion="linear", vel_gain=0.5, max_age=30,
           min_hits=1):
    """mscnn_track_params as a dict (new_thr None: high_thr)."""
    return dict(high_thr=float(high_thr), low_thr=float(low_thr), new_thr=float(high_thr if new_thr is None else new_thr),
                match_thr=float(match_thr), match_thr_low=float(match_thr_low), vel_gain=float(vel_gain),
                motion=MOTIONS.get(motion, motion), max_age=int(max_age), min_hits=int(min_hits))


def new_slot():
    """A slot after mscnn_tracks_state_reset."""
    return dict(n=0, next_id=1, frame=0, dropped=0, skipped=0, tracks=[])


def overlap_pairs(A, B):
    """r(i, j) = det_overlap<false>(A_i, B_j), [a, b] float64, the op's statements one per line; NaN where there is no pair."""
    A = np.asarray(A, np.float64).reshape(-1, 4)[:, None, :]
    B = np.asarray(B, np.float64).reshape(-1, 4)[None, :, :]
    with np.errstate(all="ignore"):
        iw = np.fmin(A[..., 0] + A[..., 2], B[..., 0] + B[..., 2]) - np.fmax(A[..., 0], B[..., 0])
        ih = np.fmin(A[..., 1] + A[..., 3], B[..., 1] + B[..., 3]) - np.fmax(A[..., 1], B[..., 1])
        o = iw * ih
        u = A[..., 2] * A[..., 3] + B[..., 2] * B[..., 3] - o
        r = o / u
        return np.where((iw <= 0) | (ih <= 0), np.nan, r)


def match_walk(r, thr, tracks, dets):
    """The literal walk: the eligible pairs of `tracks` x `dets` (index lists) in the total order larger r, lower i, lower j; a pair
    whose track and detection are both free is matched.  Returns ({i: j}, rounds = None)."""
    if not len(tracks) or not len(dets):
        return {}, None
    sub = r[np.ix_(tracks, dets)]
    with np.errstate(invalid="ignore"):
        ii, jj = np.nonzero(sub > thr)      # (a NaN is no pair)
    pairs = sorted((-float(sub[a, b]), tracks[a], dets[b]) for a, b in zip(ii.tolist(), jj.tolist()))
    ti, dj = {}, set()
    for _, i, j in pairs:
        if i not in ti and j not in dj:
            ti[i] = j
            dj.add(j)
    return ti, None


def match_rounds(r, thr, tracks, dets):
    """The same matching by rounds: every pair that is the best remaining pair of both its track and its detection is matched at once.
    At most min(tracks, detections) rounds, a bound the loop carries.  Returns ({i: j}, rounds that matched something)."""
    tfree, dfree = list(tracks), list(dets)
    ti, done = {}, 0

    def best(own, others, key):
        b = None
        for x in others:
            v = key(own, x)
            if v > thr and (b is None or v > key(own, b)):      # strict > over ascending index: the lower index among equal r
                b = x
        return b
    with np.errstate(invalid="ignore"):
        for _ in range(min(len(tracks), len(dets))):
            bd = {i: best(i, dfree, lambda i, j: r[i, j]) for i in tfree}
            bt = {j: best(j, tfree, lambda j, i: r[i, j]) for j in dfree}
            got = [(i, j) for i, j in bd.items() if j is not None and bt[j] == i]
            if not got:
                break
            done += 1
            for i, j in got:
                ti[i] = j
                tfree.remove(i)
                dfree.remove(j)
    return ti, done


def update(slot, rows, p, max_tracks, match=match_walk, trace=None):
    """One frame of one slot, in place on `slot`.  rows: [count, 5] float64 [x y w h score], or None for an overflowed segment (an
    empty frame).  Returns the frame's track ids [count] int32 (None for an overflowed segment).  trace (a list) gets one dict per
    pass: thr, r, pairs {i: j}, rounds."""
    f8 = np.float64
    slot["frame"] += 1                                                                    # step 1
    count = None if rows is None else len(rows)                                           # step 2
    rows = np.zeros((0, 5), f8) if rows is None else np.asarray(rows, f8).reshape(-1, 5)
    m = min(len(rows), MAX_DETS)
    slot["skipped"] += len(rows) - m
    B, s = rows[:m, :4], rows[:m, 4]
    with np.errstate(invalid="ignore"):
        H = [j for j in range(m) if s[j] >= p["high_thr"]]
        L = [j for j in range(m) if s[j] >= p["low_thr"] and not s[j] >= p["high_thr"]]
    tr = slot["tracks"]
    n = len(tr)
    if p["motion"] == LINEAR:                                                             # step 3
        for t in tr:
            t["box"][0] = t["box"][0] + t["vel"][0]
            t["box"][1] = t["box"][1] + t["vel"][1]
    r = overlap_pairs([t["box"] for t in tr], B) if n and m else np.zeros((n, m), f8)
    m1, k1 = match(r, p["match_thr"], list(range(n)), H)                                  # step 4
    second = [i for i in range(n) if i not in m1 and tr[i]["misses"] == 0 and tr[i]["confirmed"] != 0]
    m2, k2 = match(r, p["match_thr_low"], second, L)                                      # step 5
    if trace is not None:
        trace.append(dict(thr=p["match_thr"], r=r, pairs=dict(m1), rounds=k1, tracks=list(range(n)), dets=H))
        trace.append(dict(thr=p["match_thr_low"], r=r, pairs=dict(m2), rounds=k2, tracks=second, dets=L))
    matched = dict(m1)
    matched.update(m2)
    det_track = {j: i for i, j in matched.items()}
    alive = []
    for i, t in enumerate(tr):
        if i in matched:                                                                  # step 6
            j = matched[i]
            b = B[j]
            if p["motion"] == LINEAR:
                g = f8(t["misses"] + 1)
                dx = ((b[0] + b[2] / f8(2)) - (t["obs"][0] + t["obs"][2] / f8(2))) / g
                dy = ((b[1] + b[3] / f8(2)) - (t["obs"][1] + t["obs"][3] / f8(2))) / g
                if t["hits"] == 1:
                    t["vel"] = np.array([dx, dy], f8)
                else:
                    vx = t["vel"][0] + f8(p["vel_gain"]) * (dx - t["vel"][0])
                    vy = t["vel"][1] + f8(p["vel_gain"]) * (dy - t["vel"][1])
                    t["vel"] = np.array([vx, vy], f8)
            t["box"], t["obs"], t["score"] = b.copy(), b.copy(), f8(s[j])
            t["hits"] += 1
            t["misses"] = 0
            t["confirmed"] |= int(t["hits"] >= p["min_hits"])
            alive.append(t)
        else:                                                                             # step 7
            t["misses"] += 1
            if t["confirmed"] != 0 and t["misses"] <= p["max_age"]:
                alive.append(t)
    with np.errstate(invalid="ignore"):
        births = [j for j in H if j not in det_track and s[j] >= p["new_thr"]]             # step 8
    kept = births[:max(0, max_tracks - len(alive))]                                       # step 9
    slot["dropped"] += len(births) - len(kept)
    born = {}
    for j in kept:
        t = dict(box=B[j].copy(), obs=B[j].copy(), vel=np.zeros(2, f8), score=f8(s[j]), id=slot["next_id"], hits=1, misses=0,
                 confirmed=int(p["min_hits"] <= 1))
        slot["next_id"] += 1
        born[j] = t
        alive.append(t)
    if count is None:
        ids = None
    else:                                                                                 # step 10
        ids = np.zeros(count, np.int32)
        for j in range(m):
            t = tr[det_track[j]] if j in det_track else born.get(j)
            if t is not None and t["confirmed"] != 0:
                ids[j] = t["id"]
    slot["tracks"] = alive
    slot["n"] = len(alive)
    return ids


def run(slots, frames, p, max_tracks, match=match_walk, trace=None):
    """frames[t][k] = rows of frame t, slot k (None: overflowed).  Steps every slot through the frames; returns ids[t][k]."""
    return [[update(slots[k], fr[k], p, max_tracks, match, trace) for k in range(len(slots))] for fr in frames]


def facts(slots_before, frames, p, max_tracks, match=match_rounds):
    """The facts on the witness's own result, asserted: no track or detection is matched twice, every matched pair is over its
    threshold, ids are unique and ascending in birth order (= table order), n <= max_tracks.  Returns the most rounds a pass took."""
    import copy
    slots = copy.deepcopy(slots_before)
    most = 0
    for fr in frames:
        for k, slot in enumerate(slots):
            trace = []
            update(slot, fr[k], p, max_tracks, match, trace)
            used_t, used_d = set(), set()
            for ps in trace:
                for i, j in ps["pairs"].items():
                    assert i not in used_t and j not in used_d, "a track or a detection is matched twice"
                    assert i in ps["tracks"] and j in ps["dets"], "a pair from outside the pass's sets"
                    used_t.add(i)
                    used_d.add(j)
                    assert ps["r"][i, j] > ps["thr"], "a matched pair is not over its threshold"
                most = max(most, ps["rounds"] or 0)
            ids = [t["id"] for t in slot["tracks"]]
            assert ids == sorted(ids) and len(set(ids)) == len(ids), "ids are not unique and ascending in table order"
            assert all(0 < i < slot["next_id"] for i in ids)
            assert slot["n"] == len(slot["tracks"]) <= max_tracks
    return most


# ---- the op's buffers
def pack_layout(S, cap):
    """mscnn_multi_pack_layout_of(S, cap): byte offsets of dets and ids, the pack's bytes."""
    dets = 4 * 4 * (1 + S)
    ids = dets + max(cap, 1) * 40
    return dets, ids, (ids + max(cap, 1) * 4 + 15) // 16 * 16


def pack_bytes(frames, seg_cap, form="merge", fill=0xFF):
    """The multi pack of frames[t][k] (rows [count, 5] or None: count -1) as uint8, and the row offset of every segment.
    form "merge": every segment owns seg_cap rows at s * seg_cap, entry {count, count, s * seg_cap, 0} (the merge ops' packs);
    form "image": the K slots of frame t share {rows = seg_cap, row0 = t * seg_cap} and slot k's rows start at K * row0 + k * rows
    (mscnn_detections_multi_fwd's pack).  Rows past a count hold `fill` bytes."""
    T, K = len(frames), len(frames[0])
    S = T * K
    cap = S * seg_cap
    d_at, i_at, total = pack_layout(S, cap)
    buf = np.full(total, fill, np.uint8)
    hdr = buf[:d_at].view(np.int32)
    hdr[:4] = [S, seg_cap, cap, 0]
    rows = buf[d_at:i_at].view(np.float64).reshape(cap, 5)
    offs = []
    for t in range(T):
        for k in range(K):
            s = t * K + k
            r = frames[t][k]
            count = -1 if r is None else len(r)
            if form == "merge":
                off = s * seg_cap
                hdr[4 * (1 + s):4 * (2 + s)] = [count, max(count, 0), off, 0]
            else:
                off = K * (t * seg_cap) + k * seg_cap
                hdr[4 * (1 + s):4 * (2 + s)] = [count, seg_cap, t * seg_cap, 0]
            if r is not None and len(r):
                assert len(r) <= seg_cap
                rows[off:off + len(r)] = np.asarray(r, np.float64).reshape(-1, 5)
            offs.append(off)
    return buf, offs, cap


def state_layout(K, max_tracks):
    """mscnn_tracks_state_layout_of: (records, record, slot, total) bytes."""
    slot = 4 * HEADER_WORDS + max_tracks * RECORD_BYTES
    return 4 * HEADER_WORDS, RECORD_BYTES, slot, (K * slot + 15) // 16 * 16


def state_bytes(slots, max_tracks, base):
    """The state buffer after an update that found `base` (uint8, the buffer's bytes before) in state_out: the headers and the first
    n records of every slot are written, everything else stays."""
    rec_at, _, slot_b, total = state_layout(len(slots), max_tracks)
    out = np.array(base, np.uint8).copy()
    assert out.size == total
    for k, s in enumerate(slots):
        o = k * slot_b
        out[o:o + rec_at].view(np.int32)[:] = [s["n"], s["next_id"], s["frame"], s["dropped"], s["skipped"], 0, 0, 0]
        recs = out[o + rec_at:o + rec_at + s["n"] * RECORD_BYTES].view(RECORD)
        for i, t in enumerate(s["tracks"]):
            recs[i] = (t["box"], t["obs"], t["vel"], t["score"], t["id"], t["hits"], t["misses"], t["confirmed"])
    return out


def parse_state(buf, K, max_tracks):
    """The slots of a state buffer (uint8) as update() takes them."""
    rec_at, _, slot_b, _ = state_layout(K, max_tracks)
    buf = np.asarray(buf, np.uint8)
    slots = []
    for k in range(K):
        o = k * slot_b
        h = buf[o:o + rec_at].view(np.int32)
        n = int(h[0])
        recs = buf[o + rec_at:o + rec_at + n * RECORD_BYTES].view(RECORD)
        tracks = [dict(box=r["box"].copy(), obs=r["obs"].copy(), vel=r["vel"].copy(), score=np.float64(r["score"]), id=int(r["id"]),
                       hits=int(r["hits"]), misses=int(r["misses"]), confirmed=int(r["confirmed"])) for r in recs]
        slots.append(dict(n=n, next_id=int(h[1]), frame=int(h[2]), dropped=int(h[3]), skipped=int(h[4]), tracks=tracks))
    return slots
