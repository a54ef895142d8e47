"""The tracker behind the final stage on the GPU: mscnn_tracks_update_fwd through the HIP ABI on small synthetic packs built here
(tests/track_cases.py).  No pin on the reference, whose scripts look at no other frame: the check is tests/track_witness.py.

The op is IEEE operations only and its matching is a walk under a total order, so the bar is bit equality, not a tolerance: the whole
id buffer and the whole state -- every byte the op must write and every byte it must leave alone (both start as 0xFF poison) -- are
compared BYTE FOR BYTE with what the witness says the op writes, after every call.

Shapes, the smallest at which the kernel can go wrong -- the boundaries of det_track.hip beside the constants they come from:
  WAVE = 64                     a wave's lanes: the ballots of the compaction's ranks (tracks / detections 63 | 64 | 65)
  THREADS = kTrackThreads       1024: a thread is a track and a detection (1023 | 1024 | 1025: the last detection never enters)
  max_tracks                    the table's bound (4 against 6 births)
  K = 33                        a workgroup per slot, more slots than any launch of the final stage packs into one"""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import guarded                                   # noqa: E402
import track_cases as tc                         # noqa: E402
import track_witness as tw                       # noqa: E402


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X: torch.cuda.is_available() is False")
    from mscnn_amd import hipapi
    hipapi.lib()
    return hipapi


def cparams(hip, p):
    return hip.TrackParams(*[p[k] for k in ("high_thr", "low_thr", "new_thr", "match_thr", "match_thr_low", "vel_gain", "motion", "max_age", "min_hits")])


def fresh_state(hip, K, M):
    """A 0xFF-poisoned state, reset: exactly the headers are written."""
    nbytes = hip.lib().mscnn_tracks_state_bytes(K, M)
    assert nbytes == tw.state_layout(K, M)[3] == hip.tracks_state_layout(K, M)[3]
    state = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    hip._check(hip.lib().mscnn_tracks_state_reset(hip._dev(state), K, M, hip._stream()))
    want = tw.state_bytes([tw.new_slot() for _ in range(K)], M, np.full(nbytes, 0xFF, np.uint8))
    assert np.array_equal(state.cpu().numpy(), want), "state_reset writes the headers and nothing else"
    return state


def seg_cap_of(frames):
    return max([1] + [len(r) for fr in frames for r in fr if r is not None])


def want_ids(frames, wids, offs, cap):
    """The id buffer after a call that found it as -1 poison: a segment's first count entries, nothing else."""
    out = np.full(cap, -1, np.int32)
    K = len(frames[0])
    for t, fr in enumerate(frames):
        for k, r in enumerate(fr):
            if r is not None:
                o = offs[t * K + k]
                out[o:o + len(r)] = wids[t][k]
    return out


def call(hip, frames, p, M, state_in, slots, state_out=None, form="merge", seg_cap=None):
    """One call of the op on the pack of `frames`, checked against the witness (which steps `slots` in place): the pack unchanged, the
    id buffer and state_out byte-equal.  Returns (ids, state bytes)."""
    T, K = len(frames), len(frames[0])
    buf, offs, cap = tw.pack_bytes(frames, seg_cap_of(frames) if seg_cap is None else seg_cap, form)
    pack = torch.from_numpy(buf).cuda()
    ids = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
    out = state_in if state_out is None else state_out
    base = out.cpu().numpy()
    hip.tracks_update(cparams(hip, p), T, K, pack, cap, state_in, M, state_out, ids)
    torch.cuda.synchronize()
    wids = tw.run(slots, frames, p, M)
    got_ids, got_state = ids.cpu().numpy(), out.cpu().numpy()
    assert np.array_equal(pack.cpu().numpy(), buf), "the op wrote the pack"
    want = want_ids(frames, wids, offs, cap)
    assert np.array_equal(got_ids, want), (np.flatnonzero(got_ids != want)[:8], got_ids[got_ids != want][:8], want[got_ids != want][:8])
    ws = tw.state_bytes(slots, M, base)
    assert np.array_equal(got_state, ws), (np.flatnonzero(got_state != ws)[:8], [(s["n"], s["next_id"]) for s in slots])
    return got_ids, got_state


def stream(hip, frames, p, M, calls=None, form="merge", two=False):
    """A fresh state stepped through `frames` in calls of the given lengths (None: one call); two: state_in != state_out, the buffers
    swapped after every call.  Returns (the ids of every call, the final state's bytes, the witness's slots)."""
    K = len(frames[0])
    state, other = fresh_state(hip, K, M), (fresh_state(hip, K, M) if two else None)
    slots = [tw.new_slot() for _ in range(K)]
    all_ids, t0, final = [], 0, None
    for c in (calls or [len(frames)]):
        if two:
            before = state.clone()
            ids, final = call(hip, frames[t0:t0 + c], p, M, state, slots, state_out=other, form=form)
            assert torch.equal(state, before), "state_in was written"
            state, other = other, state
        else:
            ids, final = call(hip, frames[t0:t0 + c], p, M, state, slots, form=form)
        all_ids.append(ids)
        t0 += c
    return all_ids, final, slots


# ---- streams of six frames -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["merge", "image"])
@pytest.mark.parametrize("motion", ["none", "linear"])
def test_ids_and_state_are_byte_equal_to_the_witness_on_streams_of_six_frames(hip, motion, form):
    p = tw.params(high_thr=0.5, low_thr=0.125, match_thr=0.1, match_thr_low=0.25, motion=motion, max_age=2, min_hits=2)
    tracked = second = 0
    for seed in range(4):
        frames = tc.drift_stream(seed, T=6, K=2)
        trace = []
        tw.run([tw.new_slot(), tw.new_slot()], frames, p, 16, trace=trace)
        second += sum(len(ps["pairs"]) for ps in trace[1::2])
        ids, _, slots = stream(hip, frames, p, 16, form=form)
        tracked += int((ids[0] > 0).sum())
        assert slots[0]["n"] != slots[1]["n"] or slots[0]["next_id"] != slots[1]["next_id"], "the two slots hold the same content"
    assert tracked > 50 and second > 3, "nothing was tracked, or pass 2 matched nothing: the case shows nothing"
    stream(hip, tc.grid_stream(7, T=6, K=2), tw.params(high_thr=0.5, low_thr=0.25, match_thr=0.0, match_thr_low=0.0, motion=motion), 16, form=form)


def test_the_hand_worked_streams(hip):
    def ids_of(frames, p):
        ids, _, _ = stream(hip, frames, p, 8)
        cap = seg_cap_of(frames)
        return [ids[0][t * cap:t * cap + len(fr[0])].tolist() for t, fr in enumerate(frames)]
    low = tc.still([0.9, 0.9, 0.2, 0.9, 0.9, 0.9])
    assert ids_of(low, tw.params(high_thr=0.5, low_thr=0.1)) == [[1]] * 6
    assert ids_of(low, tw.params(high_thr=0.5, low_thr=0.5)) == [[1], [1], [0], [1], [1], [1]]
    assert ids_of(tc.moving(), tw.params(match_thr=0.2, motion="linear")) == [[1], [1], [], [1], [1], [1]]
    assert ids_of(tc.moving(), tw.params(match_thr=0.2, motion="none")) == [[1], [1], [], [2], [2], [2]]
    assert ids_of(tc.still([0.9] * 6), tw.params(min_hits=3)) == [[0], [0], [1], [1], [1], [1]]
    two = tc.rows(tc.BOX + [0.9], tc.BOX + [0.8])
    assert ids_of([[two], [two], [two[::-1]], [two], [two], [two]], tw.params()) == [[1, 2]] * 6
    max_age = 2
    gone = tc.still([0.9]) + [[tc.rows()] for _ in range(max_age + 1)]
    _, _, slots = stream(hip, gone[:-1], tw.params(max_age=max_age), 8)
    assert slots[0]["n"] == 1
    _, _, slots = stream(hip, gone, tw.params(max_age=max_age), 8)
    assert slots[0]["n"] == 0


# ---- the boundaries ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [63, 64, 65, 1023, 1024, 1025])
def test_tracks_and_detections_at_the_wave_and_the_workgroup(hip, n):
    rows = tc.crowd(n, n)
    rng = np.random.default_rng(n)
    kept = min(n, 1024)
    fewer = rows[rng.permutation(kept)[:kept - 3]]      # three tracks coast, the rest are found again in another order
    frames = [[rows], [fewer], [np.concatenate([rows[rng.permutation(kept)], rows[kept:]])]]
    ids, _, slots = stream(hip, frames, tw.params(max_age=1), 1024)
    assert slots[0]["n"] == kept and slots[0]["next_id"] == kept + 1
    assert slots[0]["skipped"] == (2 if n == 1025 else 0)
    first = ids[0][:n]
    assert sorted(first[:kept].tolist()) == list(range(1, kept + 1))
    if n == 1025:
        assert first[1024] == 0, "the 1025th detection never enters"


def test_a_crowded_table_of_1024_with_many_equal_overlaps(hip):
    rng = np.random.default_rng(5)
    frames = [[tc.grid_rows(rng, 1024, lo=0.25, side=40)] for _ in range(3)]
    p = tw.params(high_thr=0.5, low_thr=0.25, match_thr=0.2, match_thr_low=0.3, max_age=1)
    trace = []
    tw.run([tw.new_slot()], frames, p, 1024, match=tw.match_rounds, trace=trace)
    assert max(ps["rounds"] for ps in trace) >= 3 and sum(len(ps["pairs"]) for ps in trace) > 300, "the case shows nothing"
    stream(hip, frames, p, 1024)


def test_max_tracks_4_against_6_births_drops_2(hip):
    six = tc.crowd(6, 1)
    ids, _, slots = stream(hip, [[six], [six]], tw.params(), 4)
    assert slots[0]["dropped"] == 4 and slots[0]["n"] == 4      # two in each frame: the two that did not fit try again
    assert ids[0][:6].tolist() == [1, 2, 3, 4, 0, 0] and ids[0][6:12].tolist() == [1, 2, 3, 4, 0, 0]
    ids, _, slots = stream(hip, [[six]], tw.params(), 4)
    assert slots[0]["dropped"] == 2 and sorted(ids[0][:6].tolist()) == [0, 0, 1, 2, 3, 4]


@pytest.mark.parametrize("form", ["merge", "image"])
def test_33_slots(hip, form):
    frames = tc.drift_stream(9, T=3, K=33, objects=3)
    _, _, slots = stream(hip, frames, tw.params(match_thr=0.1), 8, form=form)
    assert len({(s["n"], s["next_id"]) for s in slots}) > 3


def test_an_empty_frame_and_an_overflowed_segment_in_the_middle(hip):
    frames = tc.drift_stream(2, T=6, K=2, miss=0.0)
    frames[2][0] = tc.rows()
    frames[3][1] = None
    p = tw.params(match_thr=0.1, max_age=3)
    ids, _, slots = stream(hip, frames, p, 16)      # (call() compares the whole id buffer: the overflowed segment's entries keep their -1)
    cap = seg_cap_of(frames)
    s = 3 * 2 + 1
    assert np.all(ids[0][s * cap:(s + 1) * cap] == -1)
    w = [tw.new_slot(), tw.new_slot()]
    tw.run(w, frames[:4], p, 16)
    assert w[1]["n"] > 0 and min(t["misses"] for t in w[1]["tracks"]) == 1, "the tracks coast over the overflowed segment"


def live(state, K, M):
    """The bytes of a state that mean something: the headers and the first n records, everything behind them as 0xFF.  (Records at index
    >= n are left as they were, so behind n a state holds whatever an earlier call with more tracks stored there: how the frames were
    cut into calls shows there, and nowhere else.)"""
    return tw.state_bytes(tw.parse_state(state, K, M), M, np.full(len(state), 0xFF, np.uint8))


def per_frame(all_ids, frames, calls):
    """The id entries of every (frame, slot) of a stream run in `calls`, in stream order."""
    out, t0 = [], 0
    cap_of = [seg_cap_of(frames[sum(calls[:c]):sum(calls[:c + 1])]) for c in range(len(calls))]
    for c, n in enumerate(calls):
        K = len(frames[0])
        for t in range(n):
            for k in range(K):
                r = frames[t0 + t][k]
                o = (t * K + k) * cap_of[c]
                out.append(None if r is None else all_ids[c][o:o + len(r)].tolist())
        t0 += n
    return out


def test_one_call_of_six_frames_six_calls_of_one_and_two_plus_four_give_the_same_bytes(hip):
    frames = tc.drift_stream(4, T=6, K=2)
    p = tw.params(high_thr=0.5, low_thr=0.125, match_thr=0.1, match_thr_low=0.25, max_age=1)
    runs = [[6], [1] * 6, [2, 4]]
    res = [stream(hip, frames, p, 16, calls=c) for c in runs]
    states = [live(r[1], 2, 16) for r in res]
    ids = [per_frame(r[0], frames, c) for r, c in zip(res, runs)]
    assert np.array_equal(states[0], states[1]) and np.array_equal(states[0], states[2])
    assert ids[0] == ids[1] == ids[2] and sum(len(i) for i in ids[0]) > 40


def test_in_place_and_two_buffers_give_the_same_bytes_and_twice_from_the_same_state_too(hip):
    frames = tc.drift_stream(6, T=6, K=2)
    p = tw.params(match_thr=0.1, max_age=1)
    a = stream(hip, frames, p, 16, calls=[3, 3])[1]
    b = stream(hip, frames, p, 16, calls=[3, 3], two=True)[1]      # (state_in is checked to be untouched after every call)
    assert np.array_equal(live(a, 2, 16), live(b, 2, 16))
    state = fresh_state(hip, 2, 16)
    slots = [tw.new_slot(), tw.new_slot()]
    call(hip, frames[:3], p, 16, state, slots)
    outs = []
    for _ in range(2):
        out = torch.full_like(state, 0xFF)
        outs.append(call(hip, frames[3:], p, 16, state, copy.deepcopy(slots), state_out=out))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


# ---- the buffer contract ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def arena(hip, monkeypatch):
    a = guarded.Arena("cuda")
    monkeypatch.setattr(hip, "torch", guarded.GuardedTorch(torch, a))
    yield a
    torch.cuda.synchronize()
    a.check()


def test_buffer_contract_of_the_tracker(hip, arena):
    """The pack, both states and the ids between guard bands: guards intact, the pack and state_in unwritten, of state_out and of the
    ids exactly the witness's bytes (records >= n and id entries >= count keep their poison); every refusal leaves every output poisoned."""
    frames = tc.drift_stream(1, T=4, K=2)
    p, M, T, K = tw.params(match_thr=0.1, max_age=1), 16, 4, 2
    L, Cc = hip.lib(), hip.C
    nbytes = L.mscnn_tracks_state_bytes(K, M)
    slots = [tw.new_slot(), tw.new_slot()]
    tw.run(slots, frames[:2], p, M)
    mid = tw.state_bytes(slots, M, np.full(nbytes, 0xFF, np.uint8))
    buf, offs, cap = tw.pack_bytes(frames[2:], seg_cap_of(frames) + 3)
    pack = arena.input(buf, 0xFF)
    s_in = arena.input(mid, 0xFF)
    s_out = arena.alloc(nbytes, torch.uint8)
    ids = arena.alloc(cap, torch.int32)
    hip.tracks_update(cparams(hip, p), 2, K, pack, cap, s_in, M, s_out, ids)
    torch.cuda.synchronize()
    arena.check()
    wids = tw.run(slots, frames[2:], p, M)
    assert np.array_equal(ids.cpu().numpy(), want_ids(frames[2:], wids, offs, cap))
    want = tw.state_bytes(slots, M, np.full(nbytes, 0xFF, np.uint8))
    assert np.array_equal(s_out.cpu().numpy(), want)
    rec_at, rec, slot, _ = tw.state_layout(K, M)
    assert slots[0]["n"] < M and (want[rec_at + slots[0]["n"] * rec:slot] == 0xFF).all()
    # in place, between guards
    s_io = arena.alloc(nbytes, torch.uint8)
    s_io.copy_(s_in)
    ids_b = arena.alloc(cap, torch.int32)
    hip.tracks_update(cparams(hip, p), 2, K, pack, cap, s_io, M, None, ids_b)
    torch.cuda.synchronize()
    assert torch.equal(s_io, s_out) and torch.equal(ids_b, ids)
    # refusals: nothing written
    good = {k: p[k] for k in ("high_thr", "low_thr", "new_thr", "match_thr", "match_thr_low", "vel_gain", "motion", "max_age", "min_hits")}
    out2 = arena.alloc(nbytes + 16, torch.uint8)
    ids2 = arena.alloc(cap * 4 + 16, torch.uint8)
    pack2 = arena.alloc(len(buf) + 16, torch.uint8)

    def refused(pk=pack, si=s_in, so=out2, q=ids2, T_=2, K_=K, cap_=cap, M_=M, params=True, **kw):
        tp = hip.TrackParams(*[dict(good, **kw)[k] for k in good])
        return L.mscnn_tracks_update_fwd(Cc.byref(tp) if params else None, T_, K_, None if pk is None else hip._dev(pk), cap_,
                                         None if si is None else hip._dev(si), None if so is None else hip._dev(so), M_,
                                         None if q is None else hip._dev(q), hip._stream())

    nan = float("nan")
    cases = [(dict(params=False), "null pointer"), (dict(pk=None), "null pointer"), (dict(si=None), "null pointer"), (dict(so=None), "null pointer"),
             (dict(q=None), "null pointer"), (dict(T_=0), "num_frames 0"), (dict(K_=0), "num_slots 0"), (dict(cap_=0), "cap 0"),
             (dict(T_=1 << 16, K_=1 << 10, cap_=1 << 10), "65536 frames x 1024 slots x 1024 pack rows is past 2^31 - 1"),
             (dict(M_=0), "max_tracks 0 is outside [1, 1024]"), (dict(M_=1025), "max_tracks 1025 is outside [1, 1024]"),
             (dict(high_thr=nan), "high_thr is NaN"), (dict(low_thr=nan), "low_thr is NaN"), (dict(new_thr=nan), "new_thr is NaN"),
             (dict(match_thr=nan), "match_thr nan is not inside [0, 1)"), (dict(match_thr=1.0), "match_thr 1 is not inside [0, 1)"),
             (dict(match_thr=-0.5), "match_thr -0.5 is not inside"), (dict(match_thr_low=1.5), "match_thr_low 1.5 is not inside [0, 1)"),
             (dict(match_thr_low=nan), "match_thr_low nan"), (dict(low_thr=0.75), "low_thr 0.75 is above high_thr 0.5"),
             (dict(new_thr=0.25), "new_thr 0.25 is below high_thr 0.5"), (dict(vel_gain=0.0), "vel_gain 0 is not inside (0, 1]"),
             (dict(vel_gain=1.5), "vel_gain 1.5 is not inside"), (dict(vel_gain=nan), "vel_gain nan"),
             (dict(motion=0), "motion 0 is neither 1 (none) nor 2 (linear)"), (dict(motion=3), "motion 3 is neither"),
             (dict(max_age=-1), "max_age -1"), (dict(min_hits=0), "min_hits 0"),
             (dict(pk=pack2[8:]), "pack_dev must be 16-byte aligned"), (dict(si=out2[8:]), "state_in must be 16-byte aligned"),
             (dict(so=out2[8:]), "state_out must be 16-byte aligned"), (dict(q=ids2[2:]), "track_ids_dev must be 4-byte aligned"),
             (dict(si=out2, so=out2[16:]), "state_in and state_out overlap"), (dict(si=out2[16:], so=out2), "state_in and state_out overlap")]
    for kw, text in cases:
        assert refused(**kw) == 1, kw      # MSCNN_ERR_BAD_ARG
        assert "tracks_update: " + text in L.mscnn_last_error().decode(), (kw, L.mscnn_last_error().decode())
    for kw, text in ((dict(st=None), "null state"), (dict(K_=0), "num_slots 0"), (dict(M_=1025), "max_tracks 1025 is outside [1, 1024]"),
                     (dict(st=out2[8:]), "state must be 16-byte aligned")):
        a = dict(dict(st=out2, K_=K, M_=M), **kw)
        assert L.mscnn_tracks_state_reset(None if a["st"] is None else hip._dev(a["st"]), a["K_"], a["M_"], hip._stream()) == 1
        assert "tracks_state_reset: " + text in L.mscnn_last_error().decode(), (kw, L.mscnn_last_error().decode())
    assert L.mscnn_tracks_state_bytes(0, 4) == 0 and L.mscnn_tracks_state_bytes(2, 0) == 0 and L.mscnn_tracks_state_bytes(2, 1025) == 0
    torch.cuda.synchronize()
    assert guarded.all_poison(out2) and guarded.all_poison(ids2) and guarded.all_poison(pack2)


# ---- Net level ----------------------------------------------------------------------------------------------------------------------------------
import test_gpu_seq as gq                        # noqa: E402  (clip_net, small_u8: the small synthetic frames of the Seq-NMS net tests)
from mscnn_amd import net as mnet                # noqa: E402


def flat_multi(res):
    return b"".join(np.ascontiguousarray(a).tobytes() for img in res[0] for seg in img for a in seg) + repr(res[1]).encode()


def gap_thr(scores, q):
    """A threshold in the middle of the gap between two neighbouring scores near quantile q: no score sits on it."""
    s = np.unique(np.asarray(scores, np.float64))
    i = min(max(int(q * len(s)), 1), len(s) - 1)
    return float((s[i - 1] + s[i]) / 2)


def thresholds(res):
    scores = np.concatenate([seg[0][:, 4] for img in res[0] for seg in img])
    assert len(scores) >= 4
    return gap_thr(scores, 0.5), gap_thr(scores, 0.25)


def frames_of(res):
    """A detect call's result as the witness's frames[t][k] = rows [D, 5]."""
    return [[seg[0] for seg in img] for img in res[0]]


def op_on(hip, frames, p, M, state=None):
    """The op on the pack of these frames as a batched forward writes it (the K slots of an image share their rows): (ids[t][k], state)."""
    T, K = len(frames), len(frames[0])
    cap_seg = seg_cap_of(frames)
    buf, offs, cap = tw.pack_bytes(frames, cap_seg, "image")
    state = fresh_state(hip, K, M) if state is None else state
    _, ids = hip.tracks_update(cparams(hip, p), T, K, torch.from_numpy(buf).cuda(), cap, state, M)
    ids = ids.cpu().numpy()
    return [[ids[offs[t * K + k]:offs[t * K + k] + len(frames[t][k])] for k in range(K)] for t in range(T)], state


def same_ids(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all(np.array_equal(u, v) for u, v in zip(x, y)) for x, y in zip(a, b))


def test_net_tracker_returns_the_parents_detections_and_the_ops_ids_and_state_and_off_again_nothing(hip):
    T, classes = 4, [2, 3]
    n, params, R = gq.clip_net([gq.small_u8(47, 2 * t) for t in range(T)])
    assert n.get_tracker() is None
    plain = n.detect_multi(params, classes)
    with pytest.raises(mnet.NetError, match="did not run the tracker"):
        n.detect_tracks()
    hi, lo = thresholds(plain)
    kw = dict(high_thr=hi, low_thr=lo, match_thr=0.2, match_thr_low=0.3, motion="linear", max_age=2, min_hits=1, max_tracks=64)
    n.set_tracker(**kw)
    assert n.get_tracker() == dict(kw, new_thr=hi, vel_gain=0.5)
    got = n.detect_multi(params, classes)
    assert flat_multi(got) == flat_multi(plain), "the tracker changed the detections"
    ids, state = n.detect_tracks(), n.tracker_state(raw=True)
    p = tw.params(**{k: v for k, v in kw.items() if k != "max_tracks"})
    want_ids, want_state = op_on(hip, frames_of(plain), p, 64)
    assert same_ids(ids, want_ids)
    assert np.array_equal(live(state, 2, 64), live(want_state.cpu().numpy(), 2, 64))
    seen = [set(i[k].tolist()) - {0} for i in ids for k in range(2)]
    assert any(seen[k] & seen[2 + k] for k in range(2)), "no id lives over two frames on this net: the case shows nothing"
    slots = n.tracker_state()
    assert [s["frame"] for s in slots] == [T, T] and slots[0]["n"] == len(slots[0]["tracks"]) > 0
    # a second call goes on from the committed table
    again = n.detect_multi(params, classes)
    assert flat_multi(again) == flat_multi(plain)
    want2, _ = op_on(hip, frames_of(plain), p, 64, state=want_state)
    assert same_ids(n.detect_tracks(), want2) and [s["frame"] for s in n.tracker_state()] == [2 * T, 2 * T]
    # a new stream
    n.tracker_reset()
    with pytest.raises(mnet.NetError, match="did not run the tracker"):
        n.detect_tracks()
    n.detect_multi(params, classes)
    assert same_ids(n.detect_tracks(), want_ids), "tracker_reset starts again at id 1"
    # off again
    n.set_tracker(None)
    assert n.get_tracker() is None
    assert flat_multi(n.detect_multi(params, classes)) == flat_multi(plain)
    with pytest.raises(mnet.NetError, match="did not run the tracker"):
        n.detect_tracks()
    with pytest.raises(mnet.NetError, match="the tracker is off"):
        n.tracker_state()
    with pytest.raises(mnet.NetError, match="the tracker is off"):
        n.tracker_reset()
    n.detect_image(0, 2, params[0]["ratios"], params[0]["org_hw"])      # (the single-segment forms work again)


@pytest.mark.parametrize("B", [1, 2])
def test_net_the_same_frame_fed_four_times_keeps_every_id(hip, B):
    classes = [2]
    n, params, R = gq.clip_net([gq.small_u8(47)] * B)
    plain = n.detect_multi(params, classes)
    hi, lo = thresholds(plain)
    n.set_tracker(high_thr=hi, low_thr=lo, max_tracks=256)
    per_frame = []
    for _ in range(4 // B):
        res = n.detect_multi(params, classes)
        ids = n.detect_tracks()
        per_frame += [(res[0][t][0][0], ids[t][0]) for t in range(B)]
    first = {tuple(d[:4]): int(i) for d, i in zip(*per_frame[0]) if d[4] >= hi}
    assert len(first) >= 2 and all(v > 0 for v in first.values()) and len(set(first.values())) == len(first)
    for dets, ids in per_frame[1:]:
        high = sorted(int(i) for d, i in zip(dets, ids) if d[4] >= hi)
        assert high == sorted(first.values()), "a detection over high_thr changed its id"
    assert n.tracker_state()[0]["frame"] == 4


def test_net_track_ids_persist_over_two_clips_behind_seq_nms_where_the_sequence_ids_restart(hip):
    T, classes = 2, [2]
    imgs = [gq.small_u8(47, 2 * t) for t in range(2 * T)]
    n, params, R = gq.clip_net(imgs[:T])
    n.set_seq_nms(0.5, score_thr=0.05, top_k=300)
    n.detect_merge_begin(T, 1, R)
    n.detect_merge_add(params, classes)
    hi, lo = thresholds(n.detect_merge_end())      # (of Seq-NMS's own scores on the first clip)
    n.set_tracker(high_thr=hi, low_thr=lo, match_thr=0.2, max_tracks=128)
    clips = []
    for c in range(2):
        if c:
            params = n.set_images("data", imgs[T:])
            n.forward()
        n.detect_merge_begin(T, 1, R)
        n.detect_merge_add(params, classes)
        got = n.detect_merge_end()
        clips.append((got, n.detect_merge_sequences(), n.detect_tracks()))
    # the detections are Seq-NMS's own: the tracker off gives the same rows
    n.set_tracker(None)
    n.detect_merge_begin(T, 1, R)
    n.detect_merge_add(params, classes)
    assert gq.flat(n.detect_merge_end()) == gq.flat(clips[1][0])
    tracks = [set(i for t in range(T) for i in c[2][t][0].tolist()) - {0} for c in clips]
    seqs = [[int(c[1][t][0].min()) for t in range(T) if len(c[1][t][0])] for c in clips]
    assert tracks[0] & tracks[1], "no track id lives over the clip boundary on this net: the case shows nothing"
    assert min(seqs[0]) == 0 and min(seqs[1]) == 0, "Seq-NMS's sequence ids start again in every clip"
    frames = [[c[0][0][t][0][0]] for c in clips for t in range(T)]
    want, _ = op_on(hip, frames, tw.params(high_thr=hi, low_thr=lo, match_thr=0.2), 128)
    assert same_ids([[c[2][t][0]] for c in clips for t in range(T)], want)


def test_net_tracker_refusals_name_the_setting_and_leave_the_state_as_it_was(hip):
    classes = [2, 3]
    n, params, R = gq.clip_net([gq.small_u8(47, 2 * t) for t in range(2)])
    plain = n.detect_multi(params, classes)
    hi, lo = thresholds(plain)
    for bad, text in ((dict(max_tracks=0), r"max_tracks 0 is outside \[1, 1024\]"), (dict(max_tracks=1025), "max_tracks 1025"),
                      (dict(match_thr=1.0), r"match_thr 1 is not inside \[0, 1\)"), (dict(low_thr=0.9, high_thr=0.5), "low_thr 0.9 is above high_thr 0.5"),
                      (dict(new_thr=0.1), "new_thr 0.1 is below high_thr 0.5"), (dict(vel_gain=0.0), r"vel_gain 0 is not inside \(0, 1\]"),
                      (dict(motion=3), "motion 3 is neither"), (dict(max_age=-1), "max_age -1"), (dict(min_hits=0), "min_hits 0"),
                      (dict(high_thr=float("nan")), "a NaN threshold")):
        with pytest.raises(mnet.NetError, match="set_tracker: " + text):
            n.set_tracker(**bad)
        assert n.get_tracker() is None
    with pytest.raises(mnet.NetError, match="motion 'kalman' is none of"):
        n.set_tracker(motion="kalman")
    n.set_wbf(0.55)
    with pytest.raises(mnet.NetError, match=r"set_tracker: high_thr .* while weighted boxes fusion is on \(set_wbf thr 0.55\)"):
        n.set_tracker(high_thr=hi, low_thr=lo)
    n.set_wbf(None)
    n.set_tracker(high_thr=hi, low_thr=lo, max_tracks=32)
    with pytest.raises(mnet.NetError, match=r"set_wbf: thr 0.55 while the tracker is on \(set_tracker high_thr"):
        n.set_wbf(0.55)
    assert n.get_wbf() is None
    n.detect_multi(params, classes)
    before, ids = n.tracker_state(raw=True), n.detect_tracks()
    with pytest.raises(mnet.NetError, match=r"detect_multi: 1 slots per frame, the tracker's table was made for 2"):
        n.detect_multi(params, [2])
    with pytest.raises(mnet.NetError, match="did not run the tracker"):
        n.detect_tracks()
    n.detect_merge_begin(2, 1, R)
    n.detect_merge_add(params, [2])
    with pytest.raises(mnet.NetError, match=r"detect_merge_end: 1 slots per frame, the tracker's table was made for 2"):
        n.detect_merge_end()
    one = dict(cls_id=2, ratios=params[0]["ratios"], org_hw=params[0]["org_hw"])
    for name, call_ in (("detect", lambda: n.detect(**one)), ("detect_image", lambda: n.detect_image(0, **one)),
                        ("detect_begin", lambda: n.detect_begin(R, **one)), ("detect_device", lambda: n.detect_device(R, **one)),
                        ("detect_multi_device", lambda: n.detect_multi_device(params, classes, 2 * R)),
                        ("detect_cascade", lambda: n.detect_cascade("bbox_pred", "cls_pred", "proposals_score", **one)),
                        ("detect_cascade_multi_device", lambda: n.detect_cascade_multi_device(params, [("bbox_pred", "cls_pred", "proposals_score")], classes, 2 * R))):
        with pytest.raises(mnet.NetError, match=name + r": refused while the tracker is on \(set_tracker high_thr"):
            call_()
    assert np.array_equal(n.tracker_state(raw=True), before), "a refused call stepped the tracks"
    n.detect_multi(params, classes)
    want, _ = op_on(hip, frames_of(plain) * 2, tw.params(high_thr=hi, low_thr=lo), 32)
    assert same_ids(ids + n.detect_tracks(), want)


# ---- the drivers ----------------------------------------------------------------------------------------------------------------------------------
import importlib.util                            # noqa: E402
import os                                        # noqa: E402

from mscnn_amd import zoo                        # noqa: E402

ROOT = gq.ROOT


def driver(tool, monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(ROOT, "tools"))      # (run_cascademscnn imports run_mscnn_detection, as a script's directory gives it)
    spec = importlib.util.spec_from_file_location(tool[:-3] + "_under_test", os.path.join(ROOT, "tools", tool))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    return drv


def run_main(drv, out, *args):
    assert drv.main(["--out", str(out), "--comp-id", "t", *args]) == 0
    return {f: (out / f).read_bytes() for f in sorted(os.listdir(out))}


def common_of(tool, common, tmp_path):
    if tool == "run_mscnn_detection.py":
        deploy = tmp_path / "deploy.prototxt"
        deploy.write_text(zoo.prototxt("kitti_car/mscnn-7s-576", height=96, width=320))
        return ["--prototxt", str(deploy)] + common
    return common


@pytest.mark.parametrize("tool,common", [("run_mscnn_detection.py", ["--cls-ids", "2"]), ("run_cascademscnn.py", gq.CASCADE[:-2])])
def test_driver_track_leaves_the_result_files_alone_and_writes_the_ids_detect_tracks_gave(hip, tmp_path, monkeypatch, capsys, tool, common):
    drv = driver(tool, monkeypatch)
    common = common_of(tool, common, tmp_path) + ["--synthetic", "6", "--batch", "2"]
    plain = run_main(drv, tmp_path / "plain", *common)
    seen = []
    real = mnet.Net.detect_tracks

    def spy(self):
        out = real(self)
        seen.extend(out)
        return out

    monkeypatch.setattr(mnet.Net, "detect_tracks", spy)
    tracks = tmp_path / "tracks"
    tracked = run_main(drv, tmp_path / "tracked", *common, "--track", "--track-high", "0.05", "--track-low", "0.01", "--track-match", "0.2", "--tracks-out", str(tracks))
    capsys.readouterr()
    assert tracked == plain and len(plain) == 1, "--track changed a result file"
    assert len(seen) == 6 and all(len(f) == 1 for f in seen), "one detect_tracks per group, one slot"
    name = list(plain)[0].replace("_results", "")
    assert sorted(os.listdir(tracks)) == [name]
    rows = gq.parsed((tracks / name).read_bytes(), 7)
    dets = gq.parsed(plain[list(plain)[0]], 6)
    assert len(dets) > 4 and np.array_equal(rows[:, [0, 2, 3, 4, 5, 6]], dets)
    assert np.array_equal(rows[:, 1].astype(np.int32), np.concatenate([f[0] for f in seen])) and (rows[:, 1] > 0).any()
    ids = [set(rows[rows[:, 0] == k, 1].astype(int).tolist()) - {0} for k in range(1, 7)]
    assert all(len(rows[(rows[:, 0] == k) & (rows[:, 1] > 0), 1]) == len(ids[k - 1]) for k in range(1, 7)), "an id twice in one frame"


@pytest.mark.parametrize("tool,common,fixture", [("run_mscnn_detection.py", gq.PLAIN, "plain_b1"), ("run_cascademscnn.py", gq.CASCADE, "cascade_b1")])
def test_drivers_one_frame_per_forward_still_write_the_golden_files_and_track_alone_the_same_rows(hip, tmp_path, monkeypatch, capsys, tool, common, fixture):
    """The dispatch this change touched: without the new flags one frame per forward writes tests/golden/seq_drivers/*.txt byte for byte
    (tests/test_gpu_seq.py holds all four command lines to them through the command line); --track alone sends the same frames through
    detect_multi in groups of one and writes the same file."""
    drv = driver(tool, monkeypatch)
    common = common_of(tool, list(common), tmp_path)
    want = open(os.path.join(ROOT, "tests", "golden", "seq_drivers", fixture + ".txt"), "rb").read()
    def forbidden(self, *a, **k):
        raise AssertionError("the default path reached the tracker")

    for name in ("set_tracker", "detect_tracks"):
        monkeypatch.setattr(mnet.Net, name, forbidden)
    files = run_main(drv, tmp_path / "plain", *common)
    monkeypatch.undo()
    assert len(want) > 1000 and list(files.values()) == [want]
    drv = driver(tool, monkeypatch)
    tracked = run_main(drv, tmp_path / "tracked", *common, "--track")
    capsys.readouterr()
    assert list(tracked.values()) == [want]


def test_driver_track_flag_refusals(hip, tmp_path, monkeypatch, capsys):
    drv = driver("run_mscnn_detection.py", monkeypatch)
    base = ["--model", "kitti_car/mscnn-7s-576", "--synthetic", "1"]
    for extra, text in ((["--track", "--wbf"], "--track and --wbf exclude each other"), (["--track-high", "0.7"], "belong to --track"),
                        (["--tracks-out", "x"], "belong to --track"), (["--track", "--track-low", "0.9"], "must not be above --track-high"),
                        (["--track", "--track-match", "1"], r"inside [0, 1)"), (["--track", "--proposals-only", "--proposals-out", "p"], "--track follows")):
        with pytest.raises(SystemExit):
            drv.parse_args(base + extra)
        assert text in capsys.readouterr().err
