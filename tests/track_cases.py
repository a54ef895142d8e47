"""Streams for the tracker's tests (tests/test_track_cpu.py on the witness alone, tests/test_gpu_track.py against the op): a stream is
frames[t][k] = the rows [count, 5] float64 [x y w h score] of frame t, slot k (None: an overflowed segment).  Every number is spelled
out or seeded, so the two files see the same bytes."""
import numpy as np

import track_witness as tw

BOX = [10.0, 10.0, 20.0, 20.0]


def rows(*r):
    return np.array(r, np.float64).reshape(-1, 5)


def still(scores, box=BOX):
    """One slot, one object that does not move, one frame per score."""
    return [[rows(box + [s])] for s in scores]


def moving(step=12.0, gap=2, T=6):
    """One slot, a 20 x 20 box moving `step` = 0.6 of its width per frame, score 0.9; frame `gap` has no detection at all."""
    return [[rows() if t == gap else rows([10.0 + step * t, 10.0, 20.0, 20.0, 0.9])] for t in range(T)]


def grid_rows(rng, count, lo=0.05, hi=1.0, side=12):
    """`count` boxes on a coarse grid (corners 0 .. side - 1, extents 1 .. 4): many exactly equal overlaps; scores on a grid of 1 / 16."""
    xy = rng.integers(0, side, (count, 2)).astype(np.float64)
    wh = rng.integers(1, 5, (count, 2)).astype(np.float64)
    s = rng.integers(int(lo * 16), int(hi * 16) + 1, (count, 1)).astype(np.float64) / 16.0
    return np.concatenate([xy, wh, s], axis=1)


def grid_stream(seed, T=6, K=2, counts=(0, 14), side=12):
    """K slots of different content: per frame and slot a fresh draw of lo .. hi boxes from the grid."""
    rng = np.random.default_rng(seed)
    return [[grid_rows(rng, int(rng.integers(counts[0], counts[1] + 1)), side=side) for _ in range(K)] for _ in range(T)]


def drift_stream(seed, T=6, K=2, objects=9, side=12, miss=0.2):
    """K slots; `objects` grid boxes per slot that move by whole grid steps per frame, some frames miss one, scores wander across both
    thresholds: tracks that live, coast, come back through pass 2, and die."""
    rng = np.random.default_rng(seed)
    base = [grid_rows(rng, objects + k, side=side) for k in range(K)]
    vel = [rng.integers(-1, 2, (objects + k, 2)).astype(np.float64) for k in range(K)]
    out = []
    for t in range(T):
        fr = []
        for k in range(K):
            b = base[k].copy()
            b[:, :2] += vel[k] * t
            b[:, 4] = rng.integers(1, 16, len(b)).astype(np.float64) / 16.0
            keep = rng.random(len(b)) >= miss
            fr.append(b[rng.permutation(np.flatnonzero(keep))])
        out.append(fr)
    return out


def crowd(n, seed, side=40):
    """One frame's rows for the thread-count boundaries: n distinct unit cells of a side x side lattice (no two boxes overlap: every
    detection finds exactly its own track again), scores 0.9, in a seeded order."""
    rng = np.random.default_rng(seed)
    cells = rng.permutation(side * side)[:n]
    r = np.zeros((n, 5), np.float64)
    r[:, 0], r[:, 1] = (cells % side) * 4.0, (cells // side) * 4.0
    r[:, 2:4] = 3.0
    r[:, 4] = 0.9
    return r


def witness(frames, p, max_tracks, slots=None, match=tw.match_walk):
    """(slots after the stream, ids[t][k]) from fresh slots (or the ones given, stepped in place)."""
    slots = [tw.new_slot() for _ in frames[0]] if slots is None else slots
    return slots, tw.run(slots, frames, p, max_tracks, match)
