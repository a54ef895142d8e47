"""The tracker for a batch of streams on the GPU: mscnn_tracks_update_streams_fwd and mscnn_tracks_state_reset_slots through the HIP
ABI on small synthetic packs (tests/track_cases.py), then the Net calls and the drivers' --streams.  No pin on the reference; the check
is tests/track_streams_witness.py = tests/track_witness.py run per stream on that stream's frames.

As in tests/test_gpu_track.py the bar is bit equality, no tolerance anywhere: the whole id buffer and the whole state -- every byte the
op must write and every byte it must leave alone (both start as 0xFF poison) -- are compared byte for byte with the witness after
every call, and with mscnn_tracks_update_fwd run on a stream's frames alone.

Shapes: the 12-pixel grids of track_cases, 0 to 14 rows per frame, K = 2, max_tracks 16 unless said; the boundaries are the streams'
  3 streams with 3 | 0 | 4 frames out of round-robin order     a stream without a frame, frames of a stream that are not adjacent
  33 streams x 2 slots, 256 streams x 1 slot                   more workgroups than any launch had; kTrackStreams, the bound
  max_tracks 5 (a slot of 552 bytes: not 16-byte aligned)       mscnn_tracks_state_reset_slots on a sub-block"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import guarded                                   # noqa: E402
import test_gpu_track as gt                      # noqa: E402  (cparams, fresh_state, seg_cap_of, want_ids, live: the single-stream tests' helpers)
import track_cases as tc                         # noqa: E402
import track_streams_witness as sw               # noqa: E402
import track_witness as tw                       # noqa: E402


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X: torch.cuda.is_available() is False")
    from mscnn_amd import hipapi
    hipapi.lib()
    return hipapi


P = tw.params(high_thr=0.5, low_thr=0.125, match_thr=0.1, match_thr_low=0.25, max_age=2, min_hits=2)
ORDER = [2, 0, 2, 2, 0, 2, 0]                    # three streams with 3, 0 and 4 frames, out of round-robin order


def three_streams(K=2):
    return [tc.drift_stream(21, T=3, K=K), [], tc.drift_stream(22, T=4, K=K)]


def seg_cap_all(per_stream):
    return max(gt.seg_cap_of(fr) for fr in per_stream if fr) if any(per_stream) else 1


def call(hip, per_stream, order, p, M, state_in, tables, state_out=None, form="merge", seg_cap=None):
    """One call of the streams op on the interleaved pack, checked against the witness (which steps `tables` in place): the pack
    unchanged, the id buffer and state_out byte-equal.  Returns (ids, state bytes, frames, stream_of, offs)."""
    N, K = len(tables), len(tables[0])
    buf, offs, cap, frames, stream_of = sw.pack_bytes(per_stream, order, seg_cap_all(per_stream) if seg_cap is None else seg_cap, form)
    pack = torch.from_numpy(buf).cuda()
    ids = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
    out = state_in if state_out is None else state_out
    base = out.cpu().numpy()
    hip.tracks_update_streams(gt.cparams(hip, p), len(frames), K, N, stream_of, pack, cap, state_in, M, state_out, ids)
    torch.cuda.synchronize()
    wids = sw.run(tables, frames, stream_of, p, M)
    got_ids, got_state = ids.cpu().numpy(), out.cpu().numpy()
    assert np.array_equal(pack.cpu().numpy(), buf), "the op wrote the pack"
    want = gt.want_ids(frames, wids, offs, cap)
    assert np.array_equal(got_ids, want), (np.flatnonzero(got_ids != want)[:8], got_ids[got_ids != want][:8], want[got_ids != want][:8])
    ws = sw.state_bytes(tables, M, base)
    assert np.array_equal(got_state, ws), (np.flatnonzero(got_state != ws)[:8], [[(s["n"], s["next_id"]) for s in t] for t in tables])
    return got_ids, got_state, frames, stream_of, offs


def ids_of_frames(ids, frames, offs, which):
    """The id entries of the frames `which` (their t), per slot."""
    K = len(frames[0])
    return [[None if frames[t][k] is None else ids[offs[t * K + k]:offs[t * K + k] + len(frames[t][k])].tolist() for k in range(K)] for t in which]


def alone(hip, frames, p, M, form="merge", state=None, slots=None):
    """mscnn_tracks_update_fwd on these frames in a pack of their own: (ids[t][k], state bytes)."""
    K = len(frames[0])
    state = gt.fresh_state(hip, K, M) if state is None else state
    slots = [tw.new_slot() for _ in range(K)] if slots is None else slots
    ids, st = gt.call(hip, frames, p, M, state, slots, form=form)
    _, offs, _ = tw.pack_bytes(frames, gt.seg_cap_of(frames), form)
    return ids_of_frames(ids, frames, offs, range(len(frames))), st


# ---- one stream is the old op ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["merge", "image"])
@pytest.mark.parametrize("motion", ["none", "linear"])
def test_one_stream_is_tracks_update_fwd_byte_for_byte(hip, motion, form):
    p = dict(P, motion=tw.MOTIONS[motion])
    for frames in (tc.grid_stream(7, T=6, K=2), tc.drift_stream(3, T=6, K=2)):
        buf, offs, cap = tw.pack_bytes(frames, gt.seg_cap_of(frames), form)
        pack = torch.from_numpy(buf).cuda()
        res = []
        for streams in (False, True):
            state = gt.fresh_state(hip, 2, 16)
            ids = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
            if streams:
                hip.tracks_update_streams(gt.cparams(hip, p), 6, 2, 1, [0] * 6, pack, cap, state, 16, None, ids)
            else:
                hip.tracks_update(gt.cparams(hip, p), 6, 2, pack, cap, state, 16, None, ids)
            torch.cuda.synchronize()
            res.append((ids.cpu().numpy(), state.cpu().numpy()))
        assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
        assert (res[0][0] > 0).any(), "nothing was tracked: the case shows nothing"
        call(hip, [frames], [0] * 6, p, 16, gt.fresh_state(hip, 2, 16), sw.new_tables(1, 2), form=form)      # (and the witness)


# ---- three streams with 3, 0 and 4 frames -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two", [False, True], ids=["in_place", "two_buffers"])
@pytest.mark.parametrize("form", ["merge", "image"])
def test_three_streams_interleaved_equal_each_stream_alone_and_the_stream_without_a_frame_keeps_its_block(hip, form, two):
    M, K, N = 16, 2, 3
    # a first call gives every stream, stream 1 too, tracks and a frame counter to keep
    first = [tc.drift_stream(30 + s, T=2, K=K) for s in range(N)]
    tables = sw.new_tables(N, K)
    state = gt.fresh_state(hip, N * K, M)
    _, mid, _, _, _ = call(hip, first, [1, 0, 2, 1, 2, 0], P, M, state, tables, form=form)
    assert [t[0]["frame"] for t in tables] == [2, 2, 2] and tables[1][0]["n"] > 0 and tables[1][1]["n"] > 0
    per = three_streams(K)
    out = torch.full_like(state, 0xFF) if two else None
    ids, after, frames, stream_of, offs = call(hip, per, ORDER, P, M, state, tables, state_out=out, form=form)
    if two:
        assert np.array_equal(state.cpu().numpy(), mid), "state_in was written"
    # the stream with no frame: its block as it was -- header (frame counter included) and the first n records; with two buffers
    # the records behind n keep state_out's poison
    blk = sw.block(after, 1, K, M)
    if two:
        want = tw.state_bytes(sw.parse_state(mid, N, K, M)[1], M, np.full(tw.state_layout(K, M)[3], 0xFF, np.uint8))[:len(blk)]
        assert np.array_equal(blk, want)
    else:
        assert np.array_equal(blk, sw.block(mid, 1, K, M))
    assert [s["frame"] for s in sw.parse_state(after, N, K, M)[1]] == [2, 2]
    assert [[t["misses"] for t in s["tracks"]] for s in sw.parse_state(after, N, K, M)[1]] == \
        [[t["misses"] for t in s["tracks"]] for s in sw.parse_state(mid, N, K, M)[1]], "a track of the stream without a frame aged"
    # every stream with frames: the single-stream op on that stream's frames alone, from that stream's tables of the first call
    _, where = sw.split(frames, stream_of, N)
    for s in (0, 2):
        st = gt.fresh_state(hip, K, M)
        slots = [tw.new_slot() for _ in range(K)]
        gt.call(hip, first[s], P, M, st, slots, form=form)
        want_ids, want_state = alone(hip, per[s], P, M, form=form, state=st, slots=slots)
        assert ids_of_frames(ids, frames, offs, where[s]) == want_ids
        blk = sw.block(gt.live(after, N * K, M), s, K, M)
        assert np.array_equal(blk, gt.live(want_state, K, M)[:len(blk)])
    assert (ids > 0).any(), "nothing was tracked: the case shows nothing"


# ---- composition ------------------------------------------------------------------------------------------------------------------------------------
def test_one_call_of_nine_frames_nine_calls_of_one_and_two_interleavings_leave_the_same_bytes(hip):
    M, K, N = 16, 2, 3
    per = [tc.drift_stream(40 + s, T=3, K=K) for s in range(N)]
    runs = [[[0, 1, 2, 0, 1, 2, 0, 1, 2]], [[s] for s in (0, 1, 2, 0, 1, 2, 0, 1, 2)], [[2, 2, 0, 1], [1, 0, 2, 0, 1]], [[1, 0, 0], [2, 1, 0, 2, 2, 1]]]
    states, all_ids = [], []
    for orders in runs:
        state, tables = gt.fresh_state(hip, N * K, M), sw.new_tables(N, K)
        at = [0] * N
        got = [[] for _ in range(N)]
        for order in orders:
            part = [per[s][at[s]:at[s] + order.count(s)] for s in range(N)]
            ids, final, frames, stream_of, offs = call(hip, part, order, P, M, state, tables)
            _, where = sw.split(frames, stream_of, N)
            for s in range(N):
                got[s] += ids_of_frames(ids, frames, offs, where[s])
                at[s] += order.count(s)
        assert at == [3, 3, 3]
        states.append(gt.live(final, N * K, M))
        all_ids.append(got)
    assert all(np.array_equal(states[0], s) for s in states[1:])
    assert all(all_ids[0] == i for i in all_ids[1:]) and sum(len(k) for s in all_ids[0] for f in s for k in f) > 60


# ---- many streams -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,T", [(33, 2, 2), (256, 1, 1)])
def test_33_streams_of_two_slots_and_256_streams_the_bound(hip, N, K, T):
    per = [tc.drift_stream(100 + s, T=T, K=K, objects=3) for s in range(N)]
    rng = np.random.default_rng(N)
    order = rng.permutation(np.repeat(np.arange(N), T)).tolist()
    tables = sw.new_tables(N, K)
    state = gt.fresh_state(hip, N * K, 8)
    call(hip, per, order, tw.params(match_thr=0.1), 8, state, tables)
    assert len({(t[0]["n"], t[0]["next_id"]) for t in tables}) > 2 and all(t[0]["frame"] == T for t in tables)
    if T == 1:      # 256 frames in one call is the bound too: one more frame, or one more stream, is refused (the contract test names them)
        assert len(order) == 256


def test_two_streams_fed_the_identical_frames_end_identical_and_nothing_leaks_across(hip):
    M, K = 16, 2
    frames = tc.drift_stream(5, T=4, K=K)
    tables = sw.new_tables(2, K)
    state = gt.fresh_state(hip, 2 * K, M)
    ids, after, fr, stream_of, offs = call(hip, [frames, frames], [0, 1, 1, 0, 0, 1, 1, 0], P, M, state, tables)
    _, where = sw.split(fr, stream_of, 2)
    assert ids_of_frames(ids, fr, offs, where[0]) == ids_of_frames(ids, fr, offs, where[1])
    assert np.array_equal(sw.block(after, 0, K, M), sw.block(after, 1, K, M))
    assert tables[0][0]["next_id"] > 4
    want_ids, want_state = alone(hip, frames, P, M)
    assert ids_of_frames(ids, fr, offs, where[1]) == want_ids, "ids start at 1 in every stream"
    assert np.array_equal(sw.block(gt.live(after, 2 * K, M), 1, K, M), gt.live(want_state, K, M)[:len(sw.block(after, 1, K, M))])


def test_max_tracks_4_against_6_births_in_one_stream_does_not_touch_dropped_of_the_other(hip):
    six, two_ = tc.crowd(6, 1), tc.crowd(2, 2)
    tables = sw.new_tables(2, 1)
    state = gt.fresh_state(hip, 2, 4)
    ids, _, fr, stream_of, offs = call(hip, [[[six], [six]], [[two_], [two_]]], [0, 1, 0, 1], tw.params(), 4, state, tables)
    assert tables[0][0]["dropped"] == 4 and tables[0][0]["n"] == 4
    assert tables[1][0]["dropped"] == 0 and tables[1][0]["n"] == 2 and tables[1][0]["next_id"] == 3
    assert ids_of_frames(ids, fr, offs, [0, 1, 2, 3]) == [[[1, 2, 3, 4, 0, 0]], [[1, 2]], [[1, 2, 3, 4, 0, 0]], [[1, 2]]]


# ---- mscnn_tracks_state_reset_slots -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [16, 5])
def test_reset_slots_resets_the_range_and_touches_no_other_byte(hip, M):
    N, K = 3, 2
    rec_at, rec, slot, total = tw.state_layout(N * K, M)
    assert (slot % 16 != 0) == (M == 5), "max_tracks 5: a slot of 552 bytes, 8-byte but not 16-byte aligned"
    tables = sw.new_tables(N, K)
    state = gt.fresh_state(hip, N * K, M)
    per = [tc.drift_stream(60 + s, T=2, K=K) for s in range(N)]
    _, before, _, _, _ = call(hip, per, [0, 1, 2, 2, 1, 0], tw.params(match_thr=0.1), M, state, tables)
    assert all(s["n"] > 0 for t in tables for s in t)
    hip.tracks_state_reset_slots(state, N * K, M, 1 * K, K)
    torch.cuda.synchronize()
    after = state.cpu().numpy()
    want = before.copy()
    for k in range(K, 2 * K):
        want[k * slot:k * slot + rec_at].view(np.int32)[:] = [0, 1, 0, 0, 0, 0, 0, 0]      # a fresh table: the header, no record byte
    assert np.array_equal(after, want)
    fresh = sw.block(gt.live(gt.fresh_state(hip, N * K, M).cpu().numpy(), N * K, M), 1, K, M)
    assert np.array_equal(sw.block(gt.live(after, N * K, M), 1, K, M), fresh), "the slots inside the range equal a fresh table"
    # the stream starts again at id 1, the others go on
    tables[1] = [tw.new_slot() for _ in range(K)]
    ids, _, fr, stream_of, offs = call(hip, per, [0, 1, 2, 2, 1, 0], tw.params(match_thr=0.1), M, state, tables)
    assert tables[1][0]["frame"] == 2 and tables[0][0]["frame"] == 4
    for a in ((0, 0), (N * K, 0), (2, 0)):      # an empty range anywhere inside: nothing
        hip.tracks_state_reset_slots(state, N * K, M, *a)
    hip.tracks_state_reset_slots(state, N * K, M, 0, N * K)      # the whole state is mscnn_tracks_state_reset
    torch.cuda.synchronize()
    assert np.array_equal(gt.live(state.cpu().numpy(), N * K, M), gt.live(gt.fresh_state(hip, N * K, M).cpu().numpy(), N * K, M))


# ---- the buffer contract ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def arena(hip, monkeypatch):
    a = guarded.Arena("cuda")
    monkeypatch.setattr(hip, "torch", guarded.GuardedTorch(torch, a))
    yield a
    torch.cuda.synchronize()
    a.check()


def test_buffer_contract_of_the_streams_tracker(hip, arena):
    """The pack, both states and the ids between guard bands: guards intact, the pack and state_in unwritten, of state_out and of the ids
    exactly the witness's bytes (records >= n and id entries >= count keep their poison); every refusal leaves every output poisoned."""
    M, K, N = 16, 2, 3
    L, Cc = hip.lib(), hip.C
    nbytes = L.mscnn_tracks_state_bytes(N * K, M)
    first = [tc.drift_stream(30 + s, T=2, K=K) for s in range(N)]
    tables = sw.new_tables(N, K)
    fr0, so0 = sw.interleave(first, [1, 0, 2, 1, 2, 0])
    sw.run(tables, fr0, so0, P, M)
    mid = sw.state_bytes(tables, M, np.full(nbytes, 0xFF, np.uint8))
    per = three_streams(K)
    buf, offs, cap, frames, stream_of = sw.pack_bytes(per, ORDER, seg_cap_all(per) + 3)
    T = len(frames)
    pack = arena.input(buf, 0xFF)
    s_in = arena.input(mid, 0xFF)
    s_out = arena.alloc(nbytes, torch.uint8)
    ids = arena.alloc(cap, torch.int32)
    hip.tracks_update_streams(gt.cparams(hip, P), T, K, N, stream_of, pack, cap, s_in, M, s_out, ids)
    torch.cuda.synchronize()
    arena.check()
    wids = sw.run(tables, frames, stream_of, P, M)
    assert np.array_equal(ids.cpu().numpy(), gt.want_ids(frames, wids, offs, cap))
    want = sw.state_bytes(tables, M, np.full(nbytes, 0xFF, np.uint8))
    assert np.array_equal(s_out.cpu().numpy(), want)
    rec_at, rec, slot, _ = tw.state_layout(N * K, M)
    flat = [x for t in tables for x in t]
    assert any(s["n"] < M for s in flat)
    for k, s in enumerate(flat):
        assert (want[k * slot + rec_at + s["n"] * rec:(k + 1) * slot] == 0xFF).all(), "records at index >= n keep their poison"
    s_io = arena.alloc(nbytes, torch.uint8)
    s_io.copy_(s_in)
    ids_b = arena.alloc(cap, torch.int32)
    hip.tracks_update_streams(gt.cparams(hip, P), T, K, N, stream_of, pack, cap, s_io, M, None, ids_b)
    torch.cuda.synchronize()
    assert torch.equal(ids_b, ids) and np.array_equal(gt.live(s_io.cpu().numpy(), N * K, M), gt.live(want, N * K, M))
    # refusals: nothing written
    good = {k: P[k] for k in ("high_thr", "low_thr", "new_thr", "match_thr", "match_thr_low", "vel_gain", "motion", "max_age", "min_hits")}
    out2 = arena.alloc(nbytes + 16, torch.uint8)
    ids2 = arena.alloc(cap * 4 + 16, torch.uint8)
    pack2 = arena.alloc(len(buf) + 16, torch.uint8)

    def refused(pk=pack, si=s_in, so=out2, q=ids2, T_=T, K_=K, N_=N, map_=stream_of, cap_=cap, M_=M, params=True, **kw):
        tp = hip.TrackParams(*[dict(good, **kw)[k] for k in good])
        m = None if map_ is None else np.ascontiguousarray(map_, np.int32)
        return L.mscnn_tracks_update_streams_fwd(Cc.byref(tp) if params else None, T_, K_, N_, None if m is None else m.ctypes.data_as(Cc.c_void_p),
                                                 None if pk is None else hip._dev(pk), cap_, None if si is None else hip._dev(si),
                                                 None if so is None else hip._dev(so), M_, None if q is None else hip._dev(q), hip._stream())

    nan = float("nan")
    cases = [(dict(params=False), "null pointer"), (dict(pk=None), "null pointer"), (dict(si=None), "null pointer"), (dict(so=None), "null pointer"),
             (dict(q=None), "null pointer"), (dict(T_=0), "num_frames 0"), (dict(K_=0), "num_slots 0"), (dict(cap_=0), "cap 0"),
             (dict(T_=1 << 16, K_=1 << 10, cap_=1 << 10, N_=1, map_=[0] * (1 << 16)), "65536 frames x 1024 slots x 1024 pack rows is past 2^31 - 1"),
             (dict(K_=1 << 24, N_=256, T_=1, map_=[0], cap_=1), "256 streams x 16777216 slots is past 2^31 - 1"),
             (dict(M_=0), "max_tracks 0 is outside [1, 1024]"), (dict(M_=1025), "max_tracks 1025 is outside [1, 1024]"),
             (dict(high_thr=nan), "high_thr is NaN"), (dict(low_thr=nan), "low_thr is NaN"), (dict(new_thr=nan), "new_thr is NaN"),
             (dict(match_thr=nan), "match_thr nan is not inside [0, 1)"), (dict(match_thr=1.0), "match_thr 1 is not inside [0, 1)"),
             (dict(match_thr_low=1.5), "match_thr_low 1.5 is not inside [0, 1)"), (dict(low_thr=0.75), "low_thr 0.75 is above high_thr 0.5"),
             (dict(new_thr=0.25), "new_thr 0.25 is below high_thr 0.5"), (dict(vel_gain=0.0), "vel_gain 0 is not inside (0, 1]"),
             (dict(motion=3), "motion 3 is neither"), (dict(max_age=-1), "max_age -1"), (dict(min_hits=0), "min_hits 0"),
             (dict(pk=pack2[8:]), "pack_dev must be 16-byte aligned"), (dict(si=out2[8:]), "state_in must be 16-byte aligned"),
             (dict(so=out2[8:]), "state_out must be 16-byte aligned"), (dict(q=ids2[2:]), "track_ids_dev must be 4-byte aligned"),
             (dict(si=out2, so=out2[16:]), "state_in and state_out overlap"), (dict(si=out2[16:], so=out2), "state_in and state_out overlap"),
             # the streams' own
             (dict(map_=None), "null stream_of"), (dict(N_=0), "num_streams 0 is outside [1, 256]"), (dict(N_=257), "num_streams 257 is outside [1, 256]"),
             (dict(T_=257, map_=[0, 1] * 128 + [0]), "num_frames 257 is above 256 with 3 streams"),
             (dict(map_=[2, 0, 2, 3, 0, 2, 0]), "stream_of[3] = 3 is outside [0, 3)"), (dict(map_=[2, 0, 2, 2, 0, 2, -1]), "stream_of[6] = -1 is outside [0, 3)"),
             (dict(N_=1), "stream_of[0] = 2 is outside [0, 1)")]
    for kw, text in cases:
        assert refused(**kw) == 1, kw      # MSCNN_ERR_BAD_ARG
        assert "tracks_update_streams: " + text in L.mscnn_last_error().decode(), (kw, L.mscnn_last_error().decode())
    for kw, text in ((dict(st=None), "null state"), (dict(S_=0), "num_slots_total 0"), (dict(M_=1025), "max_tracks 1025 is outside [1, 1024]"),
                     (dict(st=out2[8:]), "state must be 16-byte aligned"), (dict(first=-1), "slots [-1, -1 + 2) are outside [0, 6]"),
                     (dict(first=5), "slots [5, 5 + 2) are outside [0, 6]"), (dict(count=-1), "slots [0, 0 + -1) are outside [0, 6]"),
                     (dict(count=7), "slots [0, 0 + 7) are outside [0, 6]")):
        a = dict(dict(st=out2, S_=N * K, M_=M, first=0, count=2), **kw)
        assert L.mscnn_tracks_state_reset_slots(None if a["st"] is None else hip._dev(a["st"]), a["S_"], a["M_"], a["first"], a["count"], hip._stream()) == 1
        assert "tracks_state_reset_slots: " + text in L.mscnn_last_error().decode(), (kw, L.mscnn_last_error().decode())
    torch.cuda.synchronize()
    assert guarded.all_poison(out2) and guarded.all_poison(ids2) and guarded.all_poison(pack2)


# ---- Net level ----------------------------------------------------------------------------------------------------------------------------------
import test_gpu_seq as gq                        # noqa: E402  (clip_net, small_u8: the small synthetic frames of the Net tracker tests)
from mscnn_amd import net as mnet                # noqa: E402

CLASSES = [2, 3]
MT = 256


@pytest.fixture(scope="module")
def pair(hip):
    """A B = 2 forward of two different frames (two cameras), its untracked result and thresholds between its scores."""
    n, params, R = gq.clip_net([gq.small_u8(47), gq.small_u8(48)])
    plain = n.detect_multi(params, CLASSES)
    hi, lo = gt.thresholds(plain)
    return n, params, plain, dict(high_thr=hi, low_thr=lo, match_thr=0.2, max_tracks=MT)


def frames_of_image(res, b):
    """Image b of a detect call's result as one frame of the witness: [rows [D, 5] per slot]."""
    return [seg[0] for seg in res[0][b]]


def shown(ids):
    return [sorted(set(i.tolist()) - {0}) for i in ids]


def test_net_two_cameras_in_a_batch_of_two_keep_their_ids_and_each_starts_at_1(hip, pair):
    n, params, plain, kw = pair
    n.set_tracker(**kw, streams=2)
    with pytest.raises(mnet.NetError, match=r"detect_multi: 2 frames, the mapping of frames to the tracker's 2 streams names 0 \(mscnn_net_set_frame_streams\)"):
        n.detect_multi(params, CLASSES)
    n.set_frame_streams([0])
    with pytest.raises(mnet.NetError, match=r"detect_multi: 2 frames, the mapping of frames to the tracker's 2 streams names 1 "):
        n.detect_multi(params, CLASSES)
    n.set_frame_streams([0, 1])
    per_call = []
    for _ in range(4):
        got = n.detect_multi(params, CLASSES)
        assert gt.flat_multi(got) == gt.flat_multi(plain), "the tracker changed the detections"
        per_call.append(n.detect_tracks())
    for b in range(2):
        for k in range(2):
            first = per_call[0][b][k]
            dets = plain[0][b][k][0]
            high = dets[:, 4] >= kw["high_thr"]
            assert np.array_equal(np.sort(first[high]), np.arange(1, high.sum() + 1)), "every stream's slot starts at id 1"
            assert all(np.array_equal(c[b][k][high], first[high]) for c in per_call[1:]), "a detection over high_thr changed its id"
    assert sum(int((plain[0][b][k][0][:, 4] >= kw["high_thr"]).sum()) for b in range(2) for k in range(2)) >= 4
    state = n.tracker_state()
    assert len(state) == 2 and all(len(s) == 2 for s in state) and all(k["frame"] == 4 for s in state for k in s)
    raw = n.tracker_state(raw=True)
    # stream 1 is what a second Net tracking image 1 alone gives.  The second Net forwards the same pair, since only the same batch
    # gives image 1 the same boxes bit for bit: forwarded alone, as [image 1, image 1] or as [image 1, image 0] its boxes differ from
    # these by up to 3e-4 pixels (the ROI rows of a batch share their GEMM tiles), and a table holds its boxes.  There camera 0 is
    # silenced by a proposal_thr no score reaches, so image 1's detections are all that Net's tracker ever sees.
    m, mparams, _ = gq.clip_net([gq.small_u8(47), gq.small_u8(48)])
    mparams = [dict(mparams[0], proposal_thr=1e30), mparams[1]]
    solo = m.detect_multi(mparams, CLASSES)
    assert all(len(seg[0]) == 0 for seg in solo[0][0]), "camera 0 of the second Net still has detections"
    assert all(np.array_equal(x, y) for sa, sb in zip(solo[0][1], plain[0][1]) for x, y in zip(sa, sb)), \
        "image 1 forwarded in the second Net gives other detections than in the first: the comparison below shows nothing about the tracker"
    m.set_tracker(**kw, streams=2)
    m.set_frame_streams([0, 1])
    alone_ids = []
    for _ in range(4):
        m.detect_multi(mparams, CLASSES)
        alone_ids.append(m.detect_tracks())
    assert all(all(len(i) == 0 for i in a[0]) for a in alone_ids)
    assert gt.same_ids([c[1] for c in per_call], [a[1] for a in alone_ids])
    blk = sw.block(gt.live(raw, 4, MT), 1, 2, MT)
    mlive = gt.live(m.tracker_state(raw=True), 4, MT)
    assert np.array_equal(blk, sw.block(mlive, 1, 2, MT))
    assert all(k["n"] == 0 and k["next_id"] == 1 and k["frame"] == 4 for k in m.tracker_state()[0]), "the silenced camera's tables hold something"
    # and what mscnn_tracks_update_fwd gives on camera 1's detections alone
    want_ids, want_state = gt.op_on(hip, [frames_of_image(plain, 1)] * 4, tw.params(**{k: v for k, v in kw.items() if k != "max_tracks"}), MT)
    assert gt.same_ids([c[1] for c in per_call], want_ids)
    assert np.array_equal(blk, gt.live(want_state.cpu().numpy(), 2, MT)[:len(blk)])
    # the mapping [1, 0] swaps the blocks
    n.tracker_reset()
    n.set_frame_streams([1, 0])
    assert n.get_frame_streams() == [1, 0]
    for _ in range(4):
        n.detect_multi(params, CLASSES)
    swapped = gt.live(n.tracker_state(raw=True), 4, MT)
    straight = gt.live(raw, 4, MT)
    assert np.array_equal(sw.block(swapped, 0, 2, MT), sw.block(straight, 1, 2, MT))
    assert np.array_equal(sw.block(swapped, 1, 2, MT), sw.block(straight, 0, 2, MT))
    assert not np.array_equal(sw.block(straight, 0, 2, MT), sw.block(straight, 1, 2, MT)), "the two cameras see the same: the case shows nothing"
    n.set_tracker(None)


def test_net_tracker_reset_of_one_stream_restarts_it_at_id_1_and_the_other_keeps_its_ids(hip, pair):
    n, params, plain, kw = pair
    n.set_tracker(**dict(kw, max_age=0), streams=2)
    n.set_frame_streams([0, 1])
    n.tracker_reset(stream=1)                                # K is not fixed yet: succeeds, nothing to do
    n.detect_multi(params, CLASSES)
    first = n.detect_tracks()
    # one frame of other content: with max_age 0 every track dies and the next ids are new ones
    other = n.set_images("data", [gq.small_u8(49), gq.small_u8(50)])
    n.forward()
    n.detect_multi(other, CLASSES)
    params2 = n.set_images("data", [gq.small_u8(47), gq.small_u8(48)])
    n.forward()
    n.tracker_reset(stream=1)
    before = n.tracker_state()
    assert before[1][0]["frame"] == 2, "the reset runs in front of the next tracked call's update, not before"
    got = n.detect_multi(params2, CLASSES)
    assert gt.flat_multi(got) == gt.flat_multi(plain)
    third = n.detect_tracks()
    state = n.tracker_state()
    assert [s[0]["frame"] for s in state] == [3, 1], "stream 1 started again, stream 0 went on"
    assert gt.same_ids([third[1]], [first[1]]), "stream 1 starts again at id 1"
    assert any(state[0][k]["next_id"] > state[1][k]["next_id"] or state[0][k]["tracks"]["hits"].max(initial=0) > 1 for k in range(2)), \
        "stream 0's tables do not show their past: the case shows nothing"
    assert all(state[1][k]["tracks"]["hits"].max(initial=0) <= 1 for k in range(2)), "stream 1 did not start again"
    with pytest.raises(mnet.NetError, match=r"tracker_reset_stream: stream 2 is outside \[0, 2\)"):
        n.tracker_reset(stream=2)
    # a refused call between a reset and the next tracked call steps nothing and the reset still happens once
    n.tracker_reset(stream=0)
    keep = n.tracker_state(raw=True)
    with pytest.raises(mnet.NetError, match="1 slots per frame, the tracker's table was made for 2"):
        n.detect_multi(params2, [2])
    assert np.array_equal(n.tracker_state(raw=True), keep)
    n.detect_multi(params2, CLASSES)
    assert [s[0]["frame"] for s in n.tracker_state()] == [1, 2]
    n.set_tracker(None)


# ---- the drivers ----------------------------------------------------------------------------------------------------------------------------------
TRACK_FLAGS = ["--track", "--track-high", "0.05", "--track-low", "0.01", "--track-match", "0.2"]


def write_frames(path, frames):
    from PIL import Image
    os.makedirs(path)
    for i, f in enumerate(frames):
        Image.fromarray(f).save(os.path.join(path, f"{i:06d}.png"))
    return str(path)


@pytest.mark.parametrize("tool,common,batch", [("run_mscnn_detection.py", ["--cls-ids", "2"], 2), ("run_mscnn_detection.py", ["--cls-ids", "2"], 3),
                                               ("run_cascademscnn.py", gq.CASCADE[:-2], 2)])
def test_driver_streams_writes_per_stream_what_each_sequence_alone_gives_and_leaves_the_result_files_alone(hip, tmp_path, monkeypatch, capsys, tool, common, batch):
    """Two cameras multiplexed frame by frame; --batch 3 cuts the six frames into forwards whose mapping is [0, 1, 0] and [1, 0, 1]."""
    drv = gt.driver(tool, monkeypatch)
    common = gt.common_of(tool, list(common), tmp_path)
    seqs = [[gq.small_u8(47 + s, 2 * t) for t in range(3)] for s in range(2)]
    both = write_frames(tmp_path / "both", [seqs[i % 2][i // 2] for i in range(6)])
    plain = gt.run_main(drv, tmp_path / "plain", *common, "--images", both, "--batch", str(batch))
    tracks = tmp_path / "tracks"
    got = gt.run_main(drv, tmp_path / "streams", *common, "--images", both, "--batch", str(batch), *TRACK_FLAGS, "--streams", "2", "--tracks-out", str(tracks))
    assert got == plain and len(plain) == 1, "--streams changed a result file"
    name = list(plain)[0].replace("_results", "")
    stem = name[:-len(".txt")]
    assert sorted(os.listdir(tracks)) == [f"{stem}_stream0.txt", f"{stem}_stream1.txt"]
    dets = gq.parsed(plain[list(plain)[0]], 6)
    for s in range(2):
        one = tmp_path / f"tracks{s}"
        gt.run_main(drv, tmp_path / f"alone{s}", *common, "--images", write_frames(tmp_path / f"cam{s}", seqs[s]), "--batch", "1", *TRACK_FLAGS,
                    "--tracks-out", str(one))
        want = gq.parsed((one / name).read_bytes(), 7)
        rows = gq.parsed((tracks / f"{stem}_stream{s}.txt").read_bytes(), 7)
        # image index and track id: what --track --batch 1 writes for that camera's sequence alone, exactly
        assert np.array_equal(rows[:, :2], want[:, :2])
        # the boxes and scores: this run's own result file, exactly (a forward of one frame picks other kernels than a forward of
        # two or three and gives boxes that differ in the fifth digit -- with and without the tracker)
        own = dets[np.isin(dets[:, 0], [2 * i + s + 1 for i in range(3)])]
        assert np.array_equal(rows[:, 2:], own[:, 1:]) and np.array_equal(rows[:, 0], (own[:, 0] - 1 - s) // 2 + 1)
        assert len(rows) > 4 and (rows[:, 1] > 0).any() and set(rows[:, 0].astype(int).tolist()) <= {1, 2, 3}
    capsys.readouterr()


def test_driver_streams_flag_refusals(hip, tmp_path, monkeypatch, capsys):
    for tool, base in (("run_mscnn_detection.py", ["--model", "kitti_car/mscnn-7s-576", "--synthetic", "1"]),
                       ("run_cascademscnn.py", ["--model", "kitti_car/cascade-mscnn-7s-576-2x", "--synthetic", "1"])):
        drv = gt.driver(tool, monkeypatch)
        for extra, text in ((["--streams", "2"], "--streams 2 belongs to --track"), (["--track", "--streams", "0"], "--streams 0: 1 .. 256 streams"),
                            (["--track", "--streams", "257"], "--streams 257: 1 .. 256 streams"),
                            (["--track", "--streams", "2", "--seq-nms"], "--streams 2 and --seq-nms exclude each other")):
            with pytest.raises(SystemExit):
                drv.parse_args(base + extra)
            assert text in capsys.readouterr().err
        assert drv.parse_args(base + ["--track", "--streams", "2", "--batch", "3"]).streams == 2
        assert drv.parse_args(base + ["--track"]).streams == 1
