"""The clips the Seq-NMS tests share (tests/test_seq_cpu.py, tests/test_gpu_seq.py): one forward of T images = the T frames of a
clip, built from test_gpu_soft.Pass so that every row is a candidate and the lists come out as list = frame x K + class; and the
expectation of a run: the bytes a 0xFF-poisoned pack and sequence buffer must hold after the op, from tests/seq_witness.py.

TEST INFRASTRUCTURE ONLY."""
import numpy as np

import seq_witness as sq
import test_gpu_soft as gs

BIG = gs.BIG
LINK = 0.5


def track_frames(T, tracks=6, dup=2, lone=3, seed=0, empty=(), extra=None):
    """Per frame a [n, 4] array of integer boxes of side 32: `tracks` objects, every third starting late and every second ending
    early.  Track k stands still (k % 3 == 0), or moves 6 pixels per frame to the right (1) or, from where the track before it will
    end, to the left (2): those two CROSS in the middle of the clip, where the one suppresses the other's box and cuts its path in
    two.  Neighbouring frames of a track overlap by well over 0.5.  Each box has up to `dup` near-duplicates per frame (what a path
    box suppresses), a moving track also a newcomer now and then, 8 pixels AHEAD of it: linked to the track's next box but not to
    its last one, so the next box has two linked predecessors with different histories.  `lone` boxes per frame overlap nothing in
    any frame (paths of one frame).  empty: frames without a row.  extra: {frame: rows to pad the frame to} with further lone boxes."""
    rng = np.random.default_rng(7000 + seed)
    frames = [[] for _ in range(T)]
    for k in range(tracks):
        t0 = int(rng.integers(1, max(2, T // 2))) if k % 3 == 0 and T > 2 else 0
        t1 = int(rng.integers(t0 + 1, T)) if k % 2 == 0 and k % 3 != 2 and T > 2 else T
        vx = (0, 6, -6)[k % 3]
        x0 = 100 + 400 * (k // 3 % 8) + (6 * (T - 1) if vx < 0 else 0)
        y0 = 100 + 150 * (k // 24) + (60 if k % 3 == 0 else 0)
        for t in range(t0, t1):
            x, y = x0 + vx * t + int(rng.integers(-1, 2)), y0 + int(rng.integers(-1, 2))
            frames[t].append([x, y, 32, 32])
            for _ in range(int(rng.integers(0, dup + 1))):
                frames[t].append([x + int(rng.integers(-4, 5)), y + int(rng.integers(-4, 5)), 32, 32])
            if vx and t >= 1 and rng.integers(0, 3) == 0:
                frames[t].append([x + (8 if vx > 0 else -8), y, 32, 32])
    cell = 0
    for t in range(T):
        want = max(len(frames[t]) + lone, (extra or {}).get(t, 0))
        while len(frames[t]) < want:                          # a cell of its own, 70 pixels from the next: overlaps nothing
            frames[t].append([60 + 70 * (cell % 200), 3000 + 70 * (cell // 200), 32, 32])
            cell += 1
    return [np.zeros((0, 4)) if t in empty else np.array(f, np.float64).reshape(-1, 4) for t, f in enumerate(frames)]


def clip_pass(frames, ncls=3, seed=0):
    """The clip as ONE forward of T images (gs.Pass): image t's rows are frame t's boxes."""
    it = iter(frames)

    def boxes(n, rng):
        b = next(it)
        assert len(b) == n
        return b

    return gs.Pass(0, [len(f) for f in frames], ncls=ncls, hw=BIG, seed=seed, boxes=boxes)


_cache = {}
CLIPS = {
    # 8 frames x 2 classes
    "T8": dict(T=8, classes=[2, 3], tracks=9, dup=2, lone=3, seed=1),
    # 9 frames with an empty one in the middle: nothing links across it
    "T9_empty_4": dict(T=9, classes=[2], tracks=12, dup=2, lone=2, seed=4, empty=(4,)),
}


def clip(name=None, **kw):
    """(classes, passes, lists, T): built once per module -- the witness rows go through C's expf one by one."""
    key = name if name is not None else repr(sorted(kw.items()))
    if key not in _cache:
        kw = dict(CLIPS[name]) if name is not None else kw
        classes, T = kw.pop("classes"), kw["T"]
        p = clip_pass(track_frames(**kw), seed=kw.get("seed", 0))
        _cache[key] = (classes, [p], gs.lists_of([p], classes), T)
    return _cache[key]


def chain_cands(lists, K, k, cap=None):
    """Chain k of lists (segment = frame x K + slot): per frame the list [n, 5], None for one that overflows cap."""
    out = []
    for l in lists[k::K]:
        c = sq.candidates_of(l)[0]
        out.append(None if cap is not None and len(c) > cap else c)
    return out


def expected_of(nbytes, lists, T, cap, link_thr=LINK, nms_overlap=None, score_thr=0.001, top_k=300, rescore="avg", max_out=0):
    """(the bytes a 0xFF-poisoned pack must hold after the op, the int32 of a 0xFF-poisoned sequence buffer, per segment the witness's
    (dets, pass, row, candidates, seq) or None for an overflowed list, the trace per chain)."""
    S = len(lists)
    K = S // T
    ov = [gs.OVERLAP] * S if nms_overlap is None else list(nms_overlap)
    want = np.full(nbytes, 0xFF, np.uint8)
    wseq = np.full(S * cap, -1, np.int32)      # (0xFF poison)
    hdr, dets, tags = gs.pack_views(want, S, cap)
    hdr[0] = [S, cap, S * cap, 0]
    res, traces = [None] * S, []
    for k in range(K):
        ch = [None if sum(len(r) for r, _ in l) > cap else l for l in lists[k::K]]
        out, tr = sq.seq_chain(ch, link_thr=link_thr, nms_overlap=ov[k::K], score_thr=score_thr, top_k=top_k, rescore=sq.RESCORE[rescore],
                               max_out=max_out)
        traces.append(tr)
        for t in range(T):
            s = t * K + k
            n = sum(len(r) for r, _ in lists[s])
            if out[t] is None:
                hdr[1 + s] = [-1, n, s * cap, 0]
                continue
            d, pas, row, cands, seq = out[t]
            hdr[1 + s] = [len(d), n, s * cap, 0]
            dets[s * cap:s * cap + len(d)] = d
            tags[s * cap:s * cap + len(d)] = (pas.astype(np.int32) << 24) | row
            wseq[s * cap:s * cap + len(d)] = seq
            res[s] = out[t]
    return want, wseq, res, traces


def facts_of(lists, T, link_thr=LINK, nms_overlap=None, score_thr=0.001, top_k=300, cap=None):
    """seq_witness.seq_facts 1 .. 6 over all chains of a case."""
    S = len(lists)
    K = S // T
    ov = [gs.OVERLAP] * S if nms_overlap is None else list(nms_overlap)
    f = np.zeros(6, bool)
    for k in range(K):
        f |= np.array(sq.seq_facts(chain_cands(lists, K, k, cap), link_thr, ov[k::K], score_thr, top_k))
    return tuple(bool(v) for v in f)
