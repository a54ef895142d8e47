"""The tracker with a Kalman filter per track on the GPU: mscnn_tracks_update_kalman_fwd through the HIP ABI, the Net behind it and
both drivers.  No pin on the reference, whose scripts look at no other frame: the check is tests/track_kalman_witness.py (a), the
header's statements in float64 numpy.

The op is IEEE operations only, one rounding each, and its matching is a walk under a total order, so the bar is bit equality: the id
buffer, the state and the filter table -- every byte the op must write and every byte it must leave alone (0xFF poison) -- are
compared BYTE FOR BYTE with what the witness says, after every call.

Shapes: max_tracks 16, T = 6, K = 2 (tests/track_cases.py), min_hits 2 and max_age 2 so that tracks are born, die unconfirmed, coast and
come back inside one call -- a table grows and shrinks, which is where a record at index >= n could be touched; one case at the
bounds (max_tracks 1024, a frame of 1030 detections)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import guarded                                   # noqa: E402
import streams                                   # noqa: E402
import track_cases as tc                         # noqa: E402
import track_kalman_witness as kw                # noqa: E402
import track_streams_witness as sw               # noqa: E402
import track_witness as tw                       # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, T, K = 16, 6, 2


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X: torch.cuda.is_available() is False")
    from mscnn_amd import hipapi
    hipapi.lib()
    return hipapi


def params(**kw_):
    d = dict(high_thr=0.5, low_thr=0.125, match_thr=0.1, match_thr_low=0.25, motion="none", max_age=2, min_hits=2)
    d.update(kw_)
    return tw.params(**d)


def cparams(hip, p):
    return hip.TrackParams(*[p[k] for k in ("high_thr", "low_thr", "new_thr", "match_thr", "match_thr_low", "vel_gain", "motion", "max_age", "min_hits")])


def ckparams(hip, kp):
    return hip.TrackKalmanParams(kp["sp"], kp["sv"], kp["sa"], kp["sav"], kp["sam"], kp["freeze"])


def fresh(hip, NK, m, alloc=None):
    """A 0xFF-poisoned state, reset (exactly the headers are written), and a 0xFF-poisoned filter table."""
    sb, fb = hip.lib().mscnn_tracks_state_bytes(NK, m), hip.tracks_kalman_state_bytes(NK, m)
    assert fb == NK * m * kw.RECORD_BYTES == NK * m * hip.TRACK_KALMAN_RECORD.itemsize
    mk = alloc or (lambda n: torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda"))
    state, filt = mk(sb), mk(fb)
    hip._check(hip.lib().mscnn_tracks_state_reset(hip._dev(state), NK, m, hip._stream()))
    return state, filt


def seg_cap_of(frames):
    return max([1] + [len(r) for fr in frames for r in fr if r is not None])


def want_ids(frames, wids, offs, cap):
    out = np.full(cap, -1, np.int32)
    k_ = len(frames[0])
    for t, fr in enumerate(frames):
        for k, r in enumerate(fr):
            if r is not None:
                o = offs[t * k_ + k]
                out[o:o + len(r)] = wids[t][k]
    return out


def kcall(hip, frames, stream_of, tables, p, kp, m, state, filt, state_out=None, filt_out=None, form="merge", ids=None, seg_cap=None):
    """One call on the pack of `frames`, checked against the witness (which steps `tables` in place): the pack unchanged; ids, state_out
    and filter_out byte-equal.  Returns (ids, state bytes, filter bytes)."""
    n_streams, k_ = len(tables), len(frames[0])
    buf, offs, cap = tw.pack_bytes(frames, seg_cap_of(frames) if seg_cap is None else seg_cap, form)
    pack = torch.from_numpy(buf).cuda()
    if ids is None:
        ids = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
    so_, fo_ = (state if state_out is None else state_out), (filt if filt_out is None else filt_out)
    base_s, base_f = so_.cpu().numpy(), fo_.cpu().numpy()
    hip.tracks_update_kalman(cparams(hip, p), ckparams(hip, kp), len(frames), k_, n_streams, stream_of, pack, cap, state, filt, m,
                             state_out, filt_out, ids)
    torch.cuda.synchronize()
    wids = kw.run_streams(tables, frames, stream_of or [0] * len(frames), p, kp, m)
    flat = [slot for tab in tables for slot in tab]
    got_ids, got_s, got_f = ids.cpu().numpy()[:cap], so_.cpu().numpy(), fo_.cpu().numpy()
    assert np.array_equal(pack.cpu().numpy(), buf), "the op wrote the pack"
    want = want_ids(frames, [w if w is not None else [None] * k_ for w in wids], offs, cap)
    assert np.array_equal(got_ids, want), (np.flatnonzero(got_ids != want)[:8], got_ids[got_ids != want][:8], want[got_ids != want][:8])
    ws = tw.state_bytes(flat, m, base_s)
    assert np.array_equal(got_s, ws), ("state", np.flatnonzero(got_s != ws)[:8], [(s["n"], s["next_id"]) for s in flat])
    wf = kw.filter_bytes(flat, m, base_f)
    assert np.array_equal(got_f, wf), ("filter", np.flatnonzero(got_f != wf)[:8], [(s["n"], s["next_id"]) for s in flat])
    return got_ids, got_s, got_f


def run_stream(hip, frames, p, kp, m, calls=None, form="merge", two=False, n_streams=1, stream_of=None):
    """Fresh tables stepped through `frames` in calls of the given lengths; two: in != out for state and filter, swapped after every call."""
    k_ = len(frames[0])
    state, filt = fresh(hip, n_streams * k_, m)
    other = fresh(hip, n_streams * k_, m) if two else None
    tables = sw.new_tables(n_streams, k_)
    t0, out = 0, None
    for c in (calls or [len(frames)]):
        so = None if stream_of is None else stream_of[t0:t0 + c]
        if two:
            b_s, b_f = state.clone(), filt.clone()
            out = kcall(hip, frames[t0:t0 + c], so, tables, p, kp, m, state, filt, other[0], other[1], form=form)
            assert torch.equal(state, b_s) and torch.equal(filt, b_f), "state_in or filter_in was written"
            (state, filt), other = other, (state, filt)
        else:
            out = kcall(hip, frames[t0:t0 + c], so, tables, p, kp, m, state, filt, form=form)
        t0 += c
    return out, tables


# ---- streams of six frames -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["merge", "image"])
@pytest.mark.parametrize("two", [False, True], ids=["inplace", "two"])
@pytest.mark.parametrize("calls", [None, [1] * 6], ids=["one_call", "six_calls"])
def test_ids_state_and_filter_are_byte_equal_to_the_witness(hip, calls, two, form):
    p, kp = params(), kw.kparams()
    tracked = shrunk = 0
    for seed in range(3):
        frames = tc.drift_stream(seed, T=T, K=K)
        sizes = []
        slots = [tw.new_slot() for _ in range(K)]
        for fr in frames:
            kw.run(slots, [fr], p, kp, M)
            sizes.append(slots[0]["n"])
        shrunk += sum(1 for a, b in zip(sizes, sizes[1:]) if b < a)
        (ids, _, _), tables = run_stream(hip, frames, p, kp, M, calls=calls, form=form, two=two)
        tracked += sum(int(t["hits"] > 2) for tab in tables for s in tab for t in s["tracks"])
    assert tracked > 10 and shrunk > 0, "nothing was tracked over frames, or no table ever shrank: the case shows nothing"
    run_stream(hip, tc.grid_stream(7, T=T, K=K), params(low_thr=0.25, match_thr=0.0, match_thr_low=0.0), kp, M, calls=calls, form=form, two=two)
    run_stream(hip, tc.moving(), params(match_thr=0.2, min_hits=1), kw.kparams(freeze_lost_height=False), M, calls=calls, form=form, two=two)


def test_compaction_moves_a_filter_record_with_its_track(hip):
    """The first track of a table dies (max_age 0) while later ones live on and a birth arrives; the following frames stay byte-equal."""
    def row(x, y, w=20.0, h=30.0, s=0.9):
        return [x, y, w, h, s]
    a, b, c, d = (10.0, 10.0), (100.0, 10.0), (200.0, 40.0), (300.0, 80.0)
    frames = [[tc.rows(row(*a), row(*b), row(*c))]]
    frames += [[tc.rows(row(b[0] + 3 * t, b[1] + t), row(c[0] - 2 * t, c[1], 20.0 + t), row(d[0], d[1] + 2 * t))] for t in range(1, 5)]
    p, kp = params(max_age=0, min_hits=1, match_thr=0.3), kw.kparams()
    slots = [tw.new_slot()]
    wids = kw.run(slots, frames, p, kp, M)
    assert [w[0].tolist() for w in wids] == [[1, 2, 3]] + [[2, 3, 4]] * 4 and [t["id"] for t in slots[0]["tracks"]] == [2, 3, 4]
    for two in (False, True):
        for calls in (None, [1] * 5, [2, 3]):
            run_stream(hip, frames, p, kp, M, calls=calls, two=two)


def test_three_streams_interleaved_and_one_idle_in_a_call(hip):
    p, kp, N = params(), kw.kparams(), 3
    per = [tc.drift_stream(s, T=4, K=K) for s in (11, 12, 13)]
    for two in (False, True):
        state, filt = fresh(hip, N * K, M)
        other = fresh(hip, N * K, M) if two else (None, None)
        tables = sw.new_tables(N, K)
        frames, so = sw.interleave([f[:2] for f in per], [0, 1, 2, 2, 1, 0])
        kcall(hip, frames, so, tables, p, kp, M, state, filt, other[0], other[1])
        if two:
            (state, filt), other = other, (state, filt)
        assert all(s["n"] > 0 for s in tables[1]), "the idle stream holds no track: the case shows nothing"
        idle_before = [dict(n=s["n"], frame=s["frame"]) for s in tables[1]]
        frames, so = sw.interleave([per[0][2:], [], per[2][2:]], [2, 0, 0, 2])      # stream 1 has no frame in this call
        _, got_s, got_f = kcall(hip, frames, so, tables, p, kp, M, state, filt, other[0], other[1])
        assert idle_before == [dict(n=s["n"], frame=s["frame"]) for s in tables[1]]
        if not two:      # in place: stream 1's blocks are the bytes they were
            continue
        slot_b = tw.state_layout(1, M)[2]
        src_s, src_f = state.cpu().numpy(), filt.cpu().numpy()
        for k in range(K):
            n = tables[1][k]["n"]
            o = (K + k) * slot_b
            assert np.array_equal(got_s[o:o + 32 + n * tw.RECORD_BYTES], src_s[o:o + 32 + n * tw.RECORD_BYTES])
            o = (K + k) * M * kw.RECORD_BYTES
            assert np.array_equal(got_f[o:o + n * kw.RECORD_BYTES], src_f[o:o + n * kw.RECORD_BYTES])


def test_the_bounds_a_full_table_of_1024_and_a_frame_of_1030(hip):
    m = 1024
    first = tc.crowd(1030, 5)
    second = first.copy()
    second[:, :2] += 0.25                                     # every object moves a little
    second[5:15, 0] += 1000.0                                 # ten of them are gone, ten new ones stand elsewhere
    p, kp = params(min_hits=1, max_age=3, match_thr=0.3), kw.kparams()
    (_, _, _), tables = run_stream(hip, [[first], [second], [second]], p, kp, m, calls=[1, 2])
    s = tables[0][0]
    assert s["n"] == 1024 and s["skipped"] == 18 and s["dropped"] == 20, (s["n"], s["skipped"], s["dropped"])


def test_guard_bytes_around_the_outputs_are_untouched(hip):
    arena = guarded.Arena("cuda")
    p, kp = params(), kw.kparams()
    frames = tc.drift_stream(3, T=T, K=K)
    for two in (False, True):
        state, filt = fresh(hip, K, M, alloc=lambda n: arena.alloc(n, torch.uint8))
        other = fresh(hip, K, M, alloc=lambda n: arena.alloc(n, torch.uint8)) if two else (None, None)
        cap = T * K * seg_cap_of(frames)
        ids = arena.alloc(cap, torch.int32)
        kcall(hip, frames, None, sw.new_tables(1, K), p, kp, M, state, filt, other[0], other[1], ids=ids)
        arena.check()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_names_its_value_and_stores_nothing(hip):
    frames = tc.drift_stream(0, T=2, K=K)
    buf, offs, cap = tw.pack_bytes(frames, seg_cap_of(frames))
    pack = torch.from_numpy(buf).cuda()
    state, filt = fresh(hip, 2 * K, M)
    big = torch.full((state.numel() + filt.numel() + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    ids = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
    s0, f0 = state.clone(), filt.clone()

    def refused(match, p=None, kp=None, **over):
        a = dict(T=2, K=K, N=1, so=None, pack=pack, cap=cap, si=state, fi=filt, M=M, so_=None, fo_=None, ids=ids)
        a.update(over)
        with pytest.raises(hip.MscnnError, match=match):
            hip.tracks_update_kalman(cparams(hip, p or params()), ckparams(hip, kp or kw.kparams()), a["T"], a["K"], a["N"], a["so"], a["pack"],
                                     a["cap"], a["si"], a["fi"], a["M"], a["so_"], a["fo_"], a["ids"])
        torch.cuda.synchronize()
        assert torch.equal(state, s0) and torch.equal(filt, f0) and bool((ids == -1).all()) and guarded.all_poison(big), "a refused call stored"

    refused(r"motion 2 is not 1 \(none\)", p=params(motion="linear"))
    refused(r"motion 3 is not 1", p=dict(params(), motion=3))
    for name, field in (("std_position", "sp"), ("std_velocity", "sv"), ("std_aspect", "sa"), ("std_aspect_velocity", "sav"),
                        ("std_aspect_measure", "sam")):
        for bad, text in ((float("nan"), "nan"), (float("inf"), "inf"), (0.0, "0"), (-0.5, "-0.5")):
            refused(rf"{name} {text} is not a finite number above 0", kp=dict(kw.kparams(), **{field: np.float64(bad)}))
    refused(r"num_frames 0", T=0)
    refused(r"num_slots 0", K=0)
    refused(r"max_tracks 1025 is outside \[1, 1024\]", M=1025)
    refused(r"match_thr 1 is not inside", p=params(match_thr=1.0))
    refused(r"num_streams 257 is outside \[1, 256\]", N=257, so=[0, 0])
    refused(r"null stream_of", N=2)
    refused(r"stream_of\[1\] = 2 is outside \[0, 2\)", N=2, so=[0, 2])
    refused(r"filter_in must be 16-byte aligned", fi=big[8:8 + filt.numel()], fo_=filt)
    refused(r"filter_out must be 16-byte aligned", fo_=big[8:8 + filt.numel()])
    refused(r"state_out must be 16-byte aligned", so_=big[8:8 + state.numel()])
    refused(r"filter_in and filter_out overlap \(\d+ bytes each\) without being equal", fi=big[:filt.numel()], fo_=big[160:160 + filt.numel()])
    sb = hip.lib().mscnn_tracks_state_bytes(K, M)      # (the call's own state: one stream)
    refused(r"filter_out \(\d+ bytes\) overlaps state_out", so_=big[:sb], fo_=big[sb - 16:sb - 16 + filt.numel()])
    refused(r"filter_in \(\d+ bytes\) overlaps state_in", si=big[:sb], so_=state, fi=big[16:16 + filt.numel()], fo_=filt)
    # what the wrapper cannot send: a wrong size, null pointers
    L = hip.lib()
    tp, fp = cparams(hip, params()), ckparams(hip, kw.kparams())

    def raw(**over):
        c = hip.TracksKalmanCall(C.sizeof(hip.TracksKalmanCall), C.addressof(tp), C.addressof(fp), 2, K, 1, None, pack.data_ptr(), cap,
                                 state.data_ptr(), state.data_ptr(), filt.data_ptr(), filt.data_ptr(), M, ids.data_ptr(), hip._stream().value)
        for k, v in over.items():
            setattr(c, k, v)
        assert L.mscnn_tracks_update_kalman_fwd(C.byref(c)) != 0
        torch.cuda.synchronize()
        assert torch.equal(state, s0) and torch.equal(filt, f0) and bool((ids == -1).all())
        return L.mscnn_last_error().decode()
    assert f"size {C.sizeof(hip.TracksKalmanCall) - 8} is not sizeof(mscnn_tracks_kalman_call) = {C.sizeof(hip.TracksKalmanCall)}" in \
        raw(size=C.sizeof(hip.TracksKalmanCall) - 8)
    for field in ("filter", "filter_in", "filter_out"):
        assert raw(**{field: None}).endswith(f"null {field}")
    assert "null pointer" in raw(track=None)
    assert L.mscnn_tracks_update_kalman_fwd(None) != 0 and "null call" in L.mscnn_last_error().decode()
    assert hip.tracks_kalman_state_bytes(0, M) == 0 and hip.tracks_kalman_state_bytes(K, 1025) == 0


# ---- the stream contract -------------------------------------------------------------------------------------------------------------------------
def _stream_case():
    """The gated case of mscnn_tracks_update_kalman_fwd (tests/streams.py): six frames of two slots as two streams of three, on the
    stream the call struct names.  It stands here until tests/stream_cases.py takes it."""
    N, SEG_CAP = 2, 24
    order = [0, 1, 0, 1, 0, 1]
    cache = {}

    def gen(seed):
        if seed not in cache:
            per = [tc.drift_stream(seed, T=3, K=K), tc.drift_stream(seed + 50, T=3, K=K)]
            buf, offs, cap, frames, stream_of = sw.pack_bytes(per, order, SEG_CAP, "merge")
            cache[seed] = (dict(pack=buf), dict(frames=frames, offs=offs, cap=cap, stream_of=stream_of))
        return cache[seed]

    def run(hip, s, b):
        x = gen(1701)[1]
        state, filt = fresh(hip, N * K, M)
        ids = torch.full((x["cap"],), -1, dtype=torch.int32, device="cuda")
        hip.tracks_update_kalman(cparams(hip, params(min_hits=1)), ckparams(hip, kw.kparams()), T, K, N, x["stream_of"], b["pack"], x["cap"], state,
                                 filt, M, ids=ids)
        return [ids, state, filt]

    def check(orc, i, o):
        x = gen(1701)[1]
        tables = sw.new_tables(N, K)
        wids = kw.run_streams(tables, x["frames"], x["stream_of"], params(min_hits=1), kw.kparams(), M)
        flat = [slot for tab in tables for slot in tab]
        assert np.array_equal(o[0], want_ids(x["frames"], wids, x["offs"], x["cap"]))
        assert (o[0] > 0).sum() > 10, "nothing was tracked: the case shows nothing"
        assert np.array_equal(o[1], tw.state_bytes(flat, M, np.full(len(o[1]), 0xFF, np.uint8)))
        assert np.array_equal(o[2], kw.filter_bytes(flat, M, np.full(len(o[2]), 0xFF, np.uint8)))

    return streams.Case("tracks_kalman", ("mscnn_tracks_state_reset", "mscnn_tracks_update_kalman_fwd"), lambda seed: gen(seed)[0], run, check)


def test_gated_the_op_waits_for_nothing_and_runs_in_its_streams_order(hip):
    streams.run_gated(_stream_case(), hip, None, torch.cuda.Stream())


# ---- the Net -------------------------------------------------------------------------------------------------------------------------------------
import test_gpu_seq as gq                        # noqa: E402  (clip_net, small_u8: the small synthetic frames of the Seq-NMS net tests)
import test_gpu_track as gt                      # noqa: E402  (flat_multi, thresholds, frames_of, same_ids, live; the drivers' helpers)
from mscnn_amd import net as mnet                # noqa: E402


def kalman_op_on(hip, frames, p, kp, m, tabs=None):
    """The op on the pack of these frames as a batched forward writes it: (ids[t][k], (state, filter))."""
    T_, K_ = len(frames), len(frames[0])
    buf, offs, cap = tw.pack_bytes(frames, seg_cap_of(frames), "image")
    state, filt = fresh(hip, K_, m) if tabs is None else tabs
    _, _, ids = hip.tracks_update_kalman(cparams(hip, p), ckparams(hip, kp), T_, K_, 1, None, torch.from_numpy(buf).cuda(), cap, state, filt, m)
    ids = ids.cpu().numpy()
    return [[ids[offs[t * K_ + k]:offs[t * K_ + k] + len(frames[t][k])] for k in range(K_)] for t in range(T_)], (state, filt)


def live_filter(buf, ns, m):
    """The first n records of every table of a filter buffer."""
    recs = np.asarray(buf, np.uint8).view(kw.RECORD).reshape(len(ns), m)
    return b"".join(recs[k, :n].tobytes() for k, n in enumerate(ns))


def test_net_filter_gives_the_ops_ids_and_tables_and_off_again_what_motion_none_gave(hip):
    T_, classes, m = 4, [2, 3], 64
    n, prm, R = gq.clip_net([gq.small_u8(47, 2 * t) for t in range(T_)])
    plain = n.detect_multi(prm, classes)
    hi, lo = gt.thresholds(plain)
    kws = dict(high_thr=hi, low_thr=lo, match_thr=0.2, match_thr_low=0.3, motion="none", max_age=2, min_hits=1, max_tracks=m)
    n.set_tracker(**kws)
    assert gt.flat_multi(n.detect_multi(prm, classes)) == gt.flat_multi(plain)
    none_ids, none_state = n.detect_tracks(), n.tracker_state(raw=True)
    n.set_tracker_kalman()
    assert n.get_tracker_kalman()["std_position"] == 1 / 20
    got = n.detect_multi(prm, classes)
    assert gt.flat_multi(got) == gt.flat_multi(plain), "the filter changed the detections"
    p, kp = tw.params(**{k: v for k, v in kws.items() if k != "max_tracks"}), kw.kparams()
    want_ids, tabs = kalman_op_on(hip, gt.frames_of(plain), p, kp, m)
    ids, state, filt = n.detect_tracks(), n.tracker_state(raw=True), n.tracker_kalman_state(raw=True)
    assert gt.same_ids(ids, want_ids), "the Net's ids are not the op's"
    ns = [s["n"] for s in n.tracker_state()]
    assert sum(ns) > 0 and np.array_equal(gt.live(state, 2, m), gt.live(tabs[0].cpu().numpy(), 2, m))
    assert live_filter(filt, ns, m) == live_filter(tabs[1].cpu().numpy(), ns, m)
    assert [len(r) for r in n.tracker_kalman_state()] == ns
    seen = [set(i[k].tolist()) - {0} for i in ids for k in range(2)]
    assert any(seen[k] & seen[2 + k] for k in range(2)), "no id lives over two frames on this net: the case shows nothing"
    # a second call goes on from the committed tables
    assert gt.flat_multi(n.detect_multi(prm, classes)) == gt.flat_multi(plain)
    want2, tabs = kalman_op_on(hip, gt.frames_of(plain), p, kp, m, tabs)
    assert gt.same_ids(n.detect_tracks(), want2) and [s["frame"] for s in n.tracker_state()] == [2 * T_, 2 * T_]
    ns = [s["n"] for s in n.tracker_state()]
    assert live_filter(n.tracker_kalman_state(raw=True), ns, m) == live_filter(tabs[1].cpu().numpy(), ns, m)
    # off again: byte for byte what motion none gave
    n.set_tracker_kalman(None)
    assert n.get_tracker_kalman() is None and n.get_tracker()["motion"] == "none"
    assert gt.flat_multi(n.detect_multi(prm, classes)) == gt.flat_multi(plain)
    assert gt.same_ids(n.detect_tracks(), none_ids)
    assert np.array_equal(gt.live(n.tracker_state(raw=True), 2, m), gt.live(none_state, 2, m))      # (headers and the first n records: the rest is the buffers' past)
    with pytest.raises(mnet.NetError, match="tracker_kalman_state: the filter is off"):
        n.tracker_kalman_state()
    # set_tracker turns the filter off; the refusals
    n.set_tracker_kalman()
    n.set_tracker(**kws)
    assert n.get_tracker_kalman() is None
    n.detect_multi(prm, classes)
    assert gt.same_ids(n.detect_tracks(), none_ids)
    n.set_tracker(**dict(kws, motion="linear"))
    with pytest.raises(mnet.NetError, match=r"the tracker's motion 2 is not 1 \(none\)"):
        n.set_tracker_kalman()
    with pytest.raises(mnet.NetError, match="motion 'kalman' is none of"):
        n.set_tracker(motion="kalman")
    n.set_tracker(None)
    with pytest.raises(mnet.NetError, match="set_tracker_kalman: the tracker is off"):
        n.set_tracker_kalman()
    assert gt.flat_multi(n.detect_multi(prm, classes)) == gt.flat_multi(plain)


def test_net_filter_with_two_streams_reset_stream_and_off_while_off(hip):
    """Two cameras in one forward with the filter on: the Net's ids and both tables are the op's with the same mapping; a reset of one
    stream starts that camera again at id 1 and leaves the other's tracks and filter records alone; turning the filter off while it is
    off drops nothing."""
    T_, classes, m, N = 4, [2, 3], 64, 2
    so = [0, 1, 0, 1]
    n, prm, R = gq.clip_net([gq.small_u8(47, 2 * t) for t in range(T_)])
    plain = n.detect_multi(prm, classes)
    hi, lo = gt.thresholds(plain)
    kws = dict(high_thr=hi, low_thr=lo, match_thr=0.2, match_thr_low=0.3, motion="none", max_age=2, min_hits=1, max_tracks=m)
    n.set_tracker(streams=N, **kws)
    n.set_frame_streams(so)
    n.set_tracker_kalman()
    assert n.get_tracker_streams() == N and n.get_frame_streams() == so
    p, kp = tw.params(**{k: v for k, v in kws.items() if k != "max_tracks"}), kw.kparams()
    frames = gt.frames_of(plain)
    K_ = len(frames[0])
    buf, offs, cap = tw.pack_bytes(frames, seg_cap_of(frames), "image")
    pack = torch.from_numpy(buf).cuda()
    state, filt = fresh(hip, N * K_, m)

    def op():
        _, _, ids = hip.tracks_update_kalman(cparams(hip, p), ckparams(hip, kp), T_, K_, N, so, pack, cap, state, filt, m)
        ids = ids.cpu().numpy()
        return [[ids[offs[t * K_ + k]:offs[t * K_ + k] + len(frames[t][k])] for k in range(K_)] for t in range(T_)]

    def same_tables():
        ns = [s["n"] for tab in n.tracker_state() for s in tab]
        assert np.array_equal(gt.live(n.tracker_state(raw=True), N * K_, m), gt.live(state.cpu().numpy(), N * K_, m))
        assert live_filter(n.tracker_kalman_state(raw=True), ns, m) == live_filter(filt.cpu().numpy(), ns, m)
        return ns
    assert gt.flat_multi(n.detect_multi(prm, classes)) == gt.flat_multi(plain)
    first = op()
    assert gt.same_ids(n.detect_tracks(), first)
    ns = same_tables()
    assert all(v > 0 for v in ns[:K_]) or all(v > 0 for v in ns[K_:]), "a camera holds no track: the case shows nothing"
    assert [len(r) for tab in n.tracker_kalman_state() for r in tab] == ns
    n.tracker_reset(stream=1)
    hip.tracks_state_reset_slots(state, N * K_, m, K_, K_)
    n.detect_multi(prm, classes)
    second = op()
    got = n.detect_tracks()
    assert gt.same_ids(got, second)
    same_tables()
    assert gt.same_ids([got[1], got[3]], [first[1], first[3]]), "the reset camera does not start again at id 1"
    assert [s["frame"] for tab in n.tracker_state() for s in tab] == [4] * K_ + [2] * K_
    # off while off: the tracks live on
    n.set_tracker(**kws)
    n.detect_multi(prm, classes)
    n.set_tracker_kalman(None)
    n.detect_multi(prm, classes)
    assert [s["frame"] for s in n.tracker_state()] == [2 * T_] * K_, "turning the filter off while it was off dropped the table"


# ---- the drivers ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tool,common", [("run_mscnn_detection.py", ["--cls-ids", "2"]), ("run_cascademscnn.py", gq.CASCADE[:-2])])
def test_driver_track_motion_kalman_leaves_the_result_files_alone_and_writes_tracks(hip, tmp_path, monkeypatch, capsys, tool, common):
    drv = gt.driver(tool, monkeypatch)
    common = gt.common_of(tool, common, tmp_path) + ["--synthetic", "6", "--batch", "2"]
    plain = gt.run_main(drv, tmp_path / "plain", *common)
    called = []
    real = mnet.Net.set_tracker_kalman
    monkeypatch.setattr(mnet.Net, "set_tracker_kalman", lambda self, *a, **k: (called.append(k), real(self, *a, **k))[1])
    tracks = tmp_path / "tracks"
    tracked = gt.run_main(drv, tmp_path / "tracked", *common, "--track", "--track-high", "0.05", "--track-low", "0.01", "--track-match", "0.2",
                          "--track-motion", "kalman", "--track-kalman-pos", "0.1", "--tracks-out", str(tracks))
    capsys.readouterr()
    assert tracked == plain and len(plain) == 1, "--track-motion kalman changed a result file"
    assert called == [dict(std_position=0.1, std_velocity=1 / 160, freeze_lost_height=True)]
    name = list(plain)[0].replace("_results", "")
    assert sorted(os.listdir(tracks)) == [name]
    rows = gq.parsed((tracks / name).read_bytes(), 7)
    dets = gq.parsed(plain[list(plain)[0]], 6)
    assert len(dets) > 4 and np.array_equal(rows[:, [0, 2, 3, 4, 5, 6]], dets) and (rows[:, 1] > 0).any()
