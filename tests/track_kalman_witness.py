"""The witness of mscnn_tracks_update_kalman_fwd (include/mscnn_hip.h): two restatements.

(a) update / run / run_streams: the ten steps of tests/track_witness.py with steps 3', 6', 7', 8', 9' of the header in float64 numpy
    scalars, statement for statement (four decoupled two-state filters; p, q, r per component): the bit-for-bit check of the kernel.  A
    track is track_witness's dict plus "kf" = dict(x, v, p, q, r), each a float64 [4].
(b) Textbook: the eight-state filter written from the equations -- F, H, diagonal Q and R, S = H P H^T + R, K = P H^T S^-1,
    P - K S K^T -- on an 8 vector and an 8 x 8 matrix.  It shares no statement with (a); tests/test_track_kalman_cpu.py holds the two
    together to rounding and (b)'s cross terms to exactly 0.

A plain helper module: `import track_kalman_witness as kw`.  filter_bytes / parse_filter speak the op's filter table.
"""
import numpy as np

import track_witness as tw

f8 = np.float64
RECORD_BYTES = 160
RECORD = np.dtype([("x", "<f8", 4), ("v", "<f8", 4), ("p", "<f8", 4), ("q", "<f8", 4), ("r", "<f8", 4)])
assert RECORD.itemsize == RECORD_BYTES


def kparams(std_position=1 / 20, std_velocity=1 / 160, std_aspect=1e-2, std_aspect_velocity=1e-5, std_aspect_measure=1e-1,
            freeze_lost_height=True):
    """mscnn_track_kalman_params as a dict."""
    return dict(sp=f8(std_position), sv=f8(std_velocity), sa=f8(std_aspect), sav=f8(std_aspect_velocity), sam=f8(std_aspect_measure),
                freeze=int(bool(freeze_lost_height)))


# ---- (a) the header's statements
def measure(b):
    """z(B) = {B.x + B.w / 2, B.y + B.h / 2, B.w / B.h, B.h}."""
    with np.errstate(all="ignore"):
        return np.array([b[0] + b[2] / f8(2), b[1] + b[3] / f8(2), b[2] / b[3], b[3]], f8)


def box_of(x):
    """w = x[2] * x[3]; box = {x[0] - w / 2, x[1] - x[3] / 2, w, x[3]}."""
    with np.errstate(all="ignore"):
        w = x[2] * x[3]
        return np.array([x[0] - w / f8(2), x[1] - x[3] / f8(2), w, x[3]], f8)


def predict(kf, misses, kp):
    """Step 3' on one filter record, in place."""
    with np.errstate(all="ignore"):
        if kp["freeze"] != 0 and misses > 0:
            kf["v"][3] = f8(0)
        h = kf["x"][3]
        e = kp["sp"] * h
        g = kp["sv"] * h
        sigp = [e, e, kp["sa"], e]
        sigv = [g, g, kp["sav"], g]
        for c in range(4):
            x, v, p, q, r = kf["x"][c], kf["v"][c], kf["p"][c], kf["q"][c], kf["r"][c]
            x = x + v
            t0 = p + q
            t1 = q + r
            p = (t0 + t1) + sigp[c] * sigp[c]
            q = t1
            r = r + sigv[c] * sigv[c]
            kf["x"][c], kf["p"][c], kf["q"][c], kf["r"][c] = x, p, q, r


def correct(kf, b, kp):
    """Step 6' on one filter record with the detection b, in place."""
    with np.errstate(all="ignore"):
        z = measure(b)
        h = kf["x"][3]
        e = kp["sp"] * h
        sigm = [e, e, kp["sam"], e]
        for c in range(4):
            x, v, p, q, r = kf["x"][c], kf["v"][c], kf["p"][c], kf["q"][c], kf["r"][c]
            s = p + sigm[c] * sigm[c]
            kx = p / s
            kv = q / s
            y = z[c] - x
            x = x + kx * y
            v = v + kv * y
            r = r - kv * q
            p = p - kx * p
            q = q - kx * q
            kf["x"][c], kf["v"][c], kf["p"][c], kf["q"][c], kf["r"][c] = x, v, p, q, r


def birth(b, kp):
    """Step 8': the filter record of a track born from b."""
    with np.errstate(all="ignore"):
        h = f8(b[3])
        e = (f8(2) * kp["sp"]) * h
        g = (f8(10) * kp["sv"]) * h
        return dict(x=measure(b), v=np.zeros(4, f8), q=np.zeros(4, f8),
                    p=np.array([e * e, e * e, kp["sa"] * kp["sa"], e * e], f8),
                    r=np.array([g * g, g * g, kp["sav"] * kp["sav"], g * g], f8))


def update(slot, rows, p, kp, max_tracks, match=tw.match_walk):
    """One frame of one slot, in place: track_witness.update with the filter as the motion (p["motion"] must be NONE).  Returns the
    frame's ids."""
    assert p["motion"] == tw.NONE
    slot["frame"] += 1                                                                    # step 1
    count = None if rows is None else len(rows)                                           # step 2
    rows = np.zeros((0, 5), f8) if rows is None else np.asarray(rows, f8).reshape(-1, 5)
    m = min(len(rows), tw.MAX_DETS)
    slot["skipped"] += len(rows) - m
    B, s = rows[:m, :4], rows[:m, 4]
    with np.errstate(invalid="ignore"):
        H = [j for j in range(m) if s[j] >= p["high_thr"]]
        L = [j for j in range(m) if s[j] >= p["low_thr"] and not s[j] >= p["high_thr"]]
    tr = slot["tracks"]
    n = len(tr)
    for t in tr:                                                                          # step 3'
        predict(t["kf"], t["misses"], kp)
        t["box"] = box_of(t["kf"]["x"])
        t["vel"] = np.array([t["kf"]["v"][0], t["kf"]["v"][1]], f8)
    r = tw.overlap_pairs([t["box"] for t in tr], B) if n and m else np.zeros((n, m), f8)
    m1, _ = match(r, p["match_thr"], list(range(n)), H)                                   # step 4
    second = [i for i in range(n) if i not in m1 and tr[i]["misses"] == 0 and tr[i]["confirmed"] != 0]
    m2, _ = match(r, p["match_thr_low"], second, L)                                       # step 5
    matched = dict(m1)
    matched.update(m2)
    det_track = {j: i for i, j in matched.items()}
    alive = []
    for i, t in enumerate(tr):
        if i in matched:                                                                  # step 6'
            j = matched[i]
            correct(t["kf"], B[j], kp)
            t["box"] = box_of(t["kf"]["x"])
            t["vel"] = np.array([t["kf"]["v"][0], t["kf"]["v"][1]], f8)
            t["obs"], t["score"] = B[j].copy(), f8(s[j])
            t["hits"] += 1
            t["misses"] = 0
            t["confirmed"] |= int(t["hits"] >= p["min_hits"])
            alive.append(t)
        else:                                                                             # step 7'
            t["misses"] += 1
            if t["confirmed"] != 0 and t["misses"] <= p["max_age"]:
                alive.append(t)
    with np.errstate(invalid="ignore"):
        births = [j for j in H if j not in det_track and s[j] >= p["new_thr"]]             # step 8'
    kept = births[:max(0, max_tracks - len(alive))]                                       # step 9'
    slot["dropped"] += len(births) - len(kept)
    born = {}
    for j in kept:
        t = dict(box=B[j].copy(), obs=B[j].copy(), vel=np.zeros(2, f8), score=f8(s[j]), id=slot["next_id"], hits=1, misses=0,
                 confirmed=int(p["min_hits"] <= 1), kf=birth(B[j], kp))
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


def run(slots, frames, p, kp, max_tracks, match=tw.match_walk):
    """frames[t][k]; steps every slot through the frames; returns ids[t][k]."""
    return [[update(slots[k], fr[k], p, kp, max_tracks, match) for k in range(len(slots))] for fr in frames]


def run_streams(tables, frames, stream_of, p, kp, max_tracks, match=tw.match_walk):
    """tables[s][k] stepped through the frames of stream s (in place); ids[t][k] in call order."""
    ids = [None] * len(frames)
    for s, tab in enumerate(tables):
        for t in [t for t, o in enumerate(stream_of) if o == s]:
            ids[t] = [update(tab[k], frames[t][k], p, kp, max_tracks, match) for k in range(len(tab))]
    return ids


def any_motion(slot, rows, p, kp, max_tracks):
    """One frame under p's motion: "kalman" (p["motion"] == "kalman": the filter over motion none) or track_witness's none / linear."""
    if p["motion"] == "kalman":
        return update(slot, rows, dict(p, motion=tw.NONE), kp, max_tracks)
    return tw.update(slot, rows, p, max_tracks)


# ---- the op's filter table
def filter_bytes(slots, max_tracks, base):
    """The filter buffer after an update that found `base` (uint8) in filter_out: the first n records of every table are written."""
    out = np.array(base, np.uint8).copy()
    assert out.size == len(slots) * max_tracks * RECORD_BYTES
    for k, s in enumerate(slots):
        o = k * max_tracks * RECORD_BYTES
        recs = out[o:o + s["n"] * RECORD_BYTES].view(RECORD)
        for i, t in enumerate(s["tracks"]):
            f = t["kf"]
            recs[i] = (f["x"], f["v"], f["p"], f["q"], f["r"])
    return out


def attach_filter(slots, buf, max_tracks):
    """Gives the tracks of tw.parse_state's slots their "kf" from a filter buffer (uint8)."""
    buf = np.asarray(buf, np.uint8)
    for k, s in enumerate(slots):
        o = k * max_tracks * RECORD_BYTES
        recs = buf[o:o + s["n"] * RECORD_BYTES].view(RECORD)
        for t, r in zip(s["tracks"], recs):
            t["kf"] = dict(x=r["x"].copy(), v=r["v"].copy(), p=r["p"].copy(), q=r["q"].copy(), r=r["r"].copy())
    return slots


# ---- (b) the textbook form
class Textbook:
    """x = (cx, cy, a, h, vcx, vcy, va, vh), P 8 x 8.  F = [[I, I], [0, I]], H = [I, 0]."""
    F = np.block([[np.eye(4), np.eye(4)], [np.zeros((4, 4)), np.eye(4)]])
    H = np.block([np.eye(4), np.zeros((4, 4))])

    def __init__(self, b, kp):
        b = np.asarray(b, f8)
        h = b[3]
        self.kp = kp
        self.x = np.concatenate([[b[0] + b[2] / 2, b[1] + b[3] / 2, b[2] / b[3], h], np.zeros(4)])
        sd = [2 * kp["sp"] * h, 2 * kp["sp"] * h, kp["sa"], 2 * kp["sp"] * h,
              10 * kp["sv"] * h, 10 * kp["sv"] * h, kp["sav"], 10 * kp["sv"] * h]
        self.P = np.diag(np.square(sd))

    def predict(self, misses):
        kp = self.kp
        if kp["freeze"] and misses > 0:
            self.x[7] = 0.0
        h = self.x[3]
        Q = np.diag(np.square([kp["sp"] * h, kp["sp"] * h, kp["sa"], kp["sp"] * h, kp["sv"] * h, kp["sv"] * h, kp["sav"], kp["sv"] * h]))
        self.x = self.F @ self.x
        self.P = self.F @ self.P @ self.F.T + Q

    def correct(self, b):
        kp = self.kp
        b = np.asarray(b, f8)
        z = np.array([b[0] + b[2] / 2, b[1] + b[3] / 2, b[2] / b[3], b[3]])
        h = self.x[3]
        R = np.diag(np.square([kp["sp"] * h, kp["sp"] * h, kp["sam"], kp["sp"] * h]))
        S = self.H @ self.P @ self.H.T + R
        K = self.P @ self.H.T @ np.linalg.inv(S)
        self.x = self.x + K @ (z - self.H @ self.x)
        self.P = self.P - K @ S @ K.T

    def cross_terms(self):
        """The entries of P outside the four 2 x 2 blocks {c, c + 4}."""
        keep = np.zeros((8, 8), bool)
        for c in range(4):
            for i in (c, c + 4):
                for j in (c, c + 4):
                    keep[i, j] = True
        return self.P[~keep]
