"""The witness of mscnn_tracks_update_streams_fwd (include/mscnn_hip.h): no new algorithm.  The frames of a call are split by stream and
tests/track_witness.run steps every stream's own slots through that stream's frames.

A plain helper module beside track_witness / track_cases.  frames[t][k] as there; stream_of[t] = the stream of frame t; tables[s][k] =
the slot dict of (stream s, slot k), slot s * K + k of the state.  interleave / split, pack_bytes / parse_pack and state_bytes /
parse_state are inverse pairs (tests/test_track_streams_cpu.py holds them to that)."""
import numpy as np

import track_witness as tw


def new_tables(N, K):
    """N streams x K slots after mscnn_tracks_state_reset."""
    return [[tw.new_slot() for _ in range(K)] for _ in range(N)]


def interleave(per_stream, order):
    """per_stream[s] = that stream's frames in its own order; order = the stream of every frame of the call, in call order (stream s
    occurs len(per_stream[s]) times).  Returns (frames, stream_of)."""
    at = [0] * len(per_stream)
    frames = []
    for s in order:
        frames.append(per_stream[s][at[s]])
        at[s] += 1
    assert at == [len(f) for f in per_stream], "the order does not use every frame of every stream exactly once"
    return frames, [int(s) for s in order]


def split(frames, stream_of, N):
    """The frames of every stream in ascending t, and their t: (per_stream[s], where[s])."""
    assert len(frames) == len(stream_of) and all(0 <= s < N for s in stream_of)
    per, where = [[] for _ in range(N)], [[] for _ in range(N)]
    for t, s in enumerate(stream_of):
        per[s].append(frames[t])
        where[s].append(t)
    return per, where


def run(tables, frames, stream_of, p, max_tracks, match=tw.match_walk):
    """Steps tables[s] through the frames of stream s (in place); returns ids[t][k] in call order."""
    per, where = split(frames, stream_of, len(tables))
    ids = [None] * len(frames)
    for s, fr in enumerate(per):
        for t, i in zip(where[s], tw.run(tables[s], fr, p, max_tracks, match)):
            ids[t] = i
    return ids


def pack_bytes(per_stream, order, seg_cap, form="merge", fill=0xFF):
    """The multi pack of the interleaved frames: (buf, offs, cap, frames, stream_of).  The pack does not know about streams: it is
    track_witness.pack_bytes of the frames in call order."""
    frames, stream_of = interleave(per_stream, order)
    buf, offs, cap = tw.pack_bytes(frames, seg_cap, form, fill)
    return buf, offs, cap, frames, stream_of


def parse_pack(buf, T, K):
    """frames[t][k] of a pack track_witness.pack_bytes made (either form): rows [count, 5], None for count -1."""
    buf = np.asarray(buf, np.uint8)
    S = T * K
    hdr = buf[:16 * (1 + S)].view(np.int32)
    assert hdr[0] == S
    cap = int(hdr[2])
    d_at, i_at, _ = tw.pack_layout(S, cap)
    rows = buf[d_at:i_at].view(np.float64).reshape(cap, 5)
    frames = []
    for t in range(T):
        e0, e1 = hdr[4 * (1 + t * K):4 * (2 + t * K)], hdr[4 * (2 + t * K):4 * (3 + t * K)] if K >= 2 else None
        image = K >= 2 and e0[2] == e1[2]
        fr = []
        for k in range(K):
            e = hdr[4 * (1 + t * K + k):4 * (2 + t * K + k)]
            off = K * int(e[2]) + k * int(e[1]) if image else int(e[2])
            fr.append(None if e[0] < 0 else rows[off:off + int(e[0])].copy())
        frames.append(fr)
    return frames


def state_bytes(tables, max_tracks, base):
    """The state of N x K tables after an update that found `base` in state_out: track_witness.state_bytes of the N * K slots in
    stream-major order."""
    return tw.state_bytes([slot for tab in tables for slot in tab], max_tracks, base)


def parse_state(buf, N, K, max_tracks):
    flat = tw.parse_state(buf, N * K, max_tracks)
    return [flat[s * K:(s + 1) * K] for s in range(N)]


def block(buf, s, K, max_tracks):
    """The bytes of stream s's K slots in a state buffer."""
    slot = tw.state_layout(1, max_tracks)[2]
    return np.asarray(buf, np.uint8)[s * K * slot:(s + 1) * K * slot]
