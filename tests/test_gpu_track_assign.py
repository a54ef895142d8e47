"""The tracker's optimal assignment on the GPU: mscnn_tracks_update_assign_fwd through the HIP ABI, the Net behind it and both
drivers.  No pin on the reference, whose scripts look at no other frame: the check is tests/track_assign_witness.py, steps 4'' and
5'' of the header in Python integers.

Weights are integers and every tie is broken by a stated order, so the bar is bit equality: the id buffer, the state -- header word 5,
the search steps, included -- and with the Kalman filter the filter table, every byte the op must write and every byte it must leave
alone (0xFF poison), are compared BYTE FOR BYTE with what the witness says, after every call.

Shapes: max_tracks 16, 6 frames of 2 slots with 12 objects each (crossing pairs, low-score frames); a dense 48 x 48 cluster; one case
at the bounds (max_tracks 1024, a frame of 1030 disjoint detections: about 1024 searches of one step)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import guarded                                   # noqa: E402
import streams                                   # noqa: E402
import track_assign_witness as aw                # noqa: E402
import track_cases as tc                         # noqa: E402
import track_kalman_witness as kw                # noqa: E402
import track_streams_witness as sw               # noqa: E402
import track_witness as tw                       # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, T, K = 16, 6, 2
MOTIONS = ["none", "linear", "kalman"]


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X: torch.cuda.is_available() is False")
    from mscnn_amd import hipapi
    hipapi.lib()
    return hipapi


def setting(motion, **over):
    """(p, kp) of a motion: "kalman" is the filter over motion none."""
    d = dict(high_thr=0.5, low_thr=0.125, match_thr=0.1, match_thr_low=0.25, motion="none" if motion == "kalman" else motion, max_age=2, min_hits=2)
    d.update(over)
    return tw.params(**d), (kw.kparams() if motion == "kalman" else None)


def cparams(hip, p):
    return hip.TrackParams(*[p[k] for k in ("high_thr", "low_thr", "new_thr", "match_thr", "match_thr_low", "vel_gain", "motion", "max_age", "min_hits")])


def ckparams(hip, kp):
    return None if kp is None else hip.TrackKalmanParams(kp["sp"], kp["sv"], kp["sa"], kp["sav"], kp["sam"], kp["freeze"])


def fresh(hip, NK, m, kalman, alloc=None):
    """A 0xFF-poisoned state, reset (exactly the headers are written), and with the filter a 0xFF-poisoned filter table."""
    mk = alloc or (lambda n: torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda"))
    state = mk(hip.lib().mscnn_tracks_state_bytes(NK, m))
    filt = mk(hip.tracks_kalman_state_bytes(NK, m)) if kalman else None
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


def acall(hip, frames, stream_of, tables, p, kp, m, state, filt, state_out=None, filt_out=None, form="merge", ids=None, assign=aw.OPTIMAL):
    """One call on the pack of `frames`, checked against the witness (which steps `tables` in place): the pack unchanged; ids, state_out
    (word 5 included) and filter_out byte-equal.  Returns (ids, state bytes, filter bytes or None)."""
    n_streams, k_ = len(tables), len(frames[0])
    buf, offs, cap = tw.pack_bytes(frames, seg_cap_of(frames), form)
    pack = torch.from_numpy(buf).cuda()
    if ids is None:
        ids = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
    so_, fo_ = (state if state_out is None else state_out), (filt if filt_out is None else filt_out)
    base_s, base_f = so_.cpu().numpy(), (None if fo_ is None else fo_.cpu().numpy())
    hip.tracks_update_assign(cparams(hip, p), ckparams(hip, kp), assign, len(frames), k_, n_streams, stream_of, pack, cap, state, m,
                             filter_in=filt, state_out=state_out, filter_out=filt_out, ids=ids)
    torch.cuda.synchronize()
    wids = aw.run_streams(tables, frames, stream_of or [0] * len(frames), p, m, kp, assign)
    flat = [slot for tab in tables for slot in tab]
    got_ids, got_s = ids.cpu().numpy()[:cap], so_.cpu().numpy()
    assert np.array_equal(pack.cpu().numpy(), buf), "the op wrote the pack"
    want = want_ids(frames, [w if w is not None else [None] * k_ for w in wids], offs, cap)
    assert np.array_equal(got_ids, want), (np.flatnonzero(got_ids != want)[:8], got_ids[got_ids != want][:8], want[got_ids != want][:8])
    ws = aw.state_bytes(flat, m, base_s, assign)
    assert np.array_equal(got_s, ws), ("state", np.flatnonzero(got_s != ws)[:8], aw.steps_of(got_s, len(flat), m), [s.get("steps") for s in flat])
    got_f = None
    if kp is not None:
        got_f = fo_.cpu().numpy()
        wf = kw.filter_bytes(flat, m, base_f)
        assert np.array_equal(got_f, wf), ("filter", np.flatnonzero(got_f != wf)[:8])
    return got_ids, got_s, got_f


def run_stream(hip, frames, p, kp, m, calls=None, form="merge", two=False, assign=aw.OPTIMAL):
    """Fresh tables stepped through `frames` in calls of the given lengths; two: in != out for state and filter, swapped after every call."""
    k_ = len(frames[0])
    state, filt = fresh(hip, k_, m, kp is not None)
    other = fresh(hip, k_, m, kp is not None) if two else None
    tables = sw.new_tables(1, k_)
    t0, out = 0, None
    for c in (calls or [len(frames)]):
        if two:
            b_s, b_f = state.clone(), (None if filt is None else filt.clone())
            out = acall(hip, frames[t0:t0 + c], None, tables, p, kp, m, state, filt, other[0], other[1], form=form, assign=assign)
            assert torch.equal(state, b_s) and (filt is None or torch.equal(filt, b_f)), "state_in or filter_in was written"
            (state, filt), other = other, (state, filt)
        else:
            out = acall(hip, frames[t0:t0 + c], None, tables, p, kp, m, state, filt, form=form, assign=assign)
        t0 += c
    return out, tables


# ---- the scene: 12 objects per slot over six frames ----------------------------------------------------------------------------------------------
def scene(seed=0, T_=T, K_=K):
    """Per slot four pairs of 30 x 40 boxes that cross each other (6 px per frame towards each other, 4 px apart in y) and four single
    boxes; every object's score drops under high_thr in some frames (pass 2), a single one is missing in one frame."""
    rng = np.random.default_rng(seed)
    frames = []
    low = rng.integers(0, T_, size=(K_, 12))
    for t in range(T_):
        fr = []
        for k in range(K_):
            rows = []
            for pr in range(4):
                x0, y0 = 120.0 * pr + 3.0 * k, 10.0 + 7.0 * pr
                rows.append([x0 + 6.0 * t, y0, 30.0, 40.0])
                rows.append([x0 + 30.0 - 6.0 * t, y0 + 4.0, 30.0, 40.0])
            for s in range(4):
                rows.append([100.0 * s + 2.0 * t, 200.0 + 3.0 * k, 24.0, 24.0])
            rows = [r + [0.25 if (low[k, o] == t and t > 0) else 0.9] for o, r in enumerate(rows)]
            if t == 3:
                del rows[9 + k]
            fr.append(np.array(rows)[rng.permutation(len(rows))])
        frames.append(fr)
    return frames


@pytest.fixture(scope="module")
def scene_facts():
    """On the witness: pass 2 matches something and a search is longer than one step, under every motion."""
    frames = scene()
    for motion in MOTIONS:
        p, kp = setting(motion)
        long_search = second = 0

        def match(r, thr, tracks, dets):
            nonlocal long_search, second
            pairs, steps = aw.match_optimal(r, thr, tracks, dets)
            with np.errstate(invalid="ignore"):
                rows = sum(1 for i in tracks if any(r[i, j] > thr for j in dets))
            long_search += steps > rows
            second += len(pairs) if thr == p["match_thr_low"] else 0
            return pairs, steps
        slots = [tw.new_slot() for _ in range(K)]
        for fr in frames:
            for k in range(K):
                tw.update(slots[k], fr[k], p, M, match) if kp is None else kw.update(slots[k], fr[k], p, kp, M, match)
        assert long_search > 0 and second > 0, (motion, long_search, second)
        assert all(len(s["tracks"]) >= 11 for s in slots)
    return frames


@pytest.mark.parametrize("motion", MOTIONS)
@pytest.mark.parametrize("form", ["merge", "image"])
@pytest.mark.parametrize("two", [False, True], ids=["inplace", "two"])
@pytest.mark.parametrize("calls", [None, [1] * 6], ids=["one_call", "six_calls"])
def test_ids_state_steps_and_filter_are_byte_equal_to_the_witness(hip, scene_facts, calls, two, form, motion):
    p, kp = setting(motion)
    (_, got_s, _), tables = run_stream(hip, scene_facts, p, kp, M, calls=calls, form=form, two=two)
    steps = aw.steps_of(got_s, K, M)
    assert steps == [s["steps"] for s in tables[0]] and min(steps) > 40, steps
    if calls is None and not two and form == "merge":      # more streams of other kinds: tables that shrink, exactly equal overlaps
        run_stream(hip, tc.drift_stream(1, T=T, K=K), p, kp, M)
        run_stream(hip, tc.grid_stream(7, T=T, K=K), setting(motion, low_thr=0.25, match_thr=0.0, match_thr_low=0.0)[0], kp, M)


@pytest.mark.parametrize("motion", ["linear", "kalman"])
def test_assign_greedy_is_the_existing_op_byte_for_byte(hip, scene_facts, motion):
    p, kp = setting(motion)
    frames = scene_facts
    buf, offs, cap = tw.pack_bytes(frames, seg_cap_of(frames))
    pack = torch.from_numpy(buf).cuda()
    out = []
    for new in (False, True):
        state, filt = fresh(hip, K, M, kp is not None)
        ids = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
        for _ in range(2):      # (a second call goes on from the first one's tables)
            if new:
                hip.tracks_update_assign(cparams(hip, p), ckparams(hip, kp), "greedy", T, K, 1, None, pack, cap, state, M, filter_in=filt, ids=ids)
            elif kp is None:
                hip.tracks_update_streams(cparams(hip, p), T, K, 1, [0] * T, pack, cap, state, M, ids=ids)
            else:
                hip.tracks_update_kalman(cparams(hip, p), ckparams(hip, kp), T, K, 1, None, pack, cap, state, filt, M, ids=ids)
        torch.cuda.synchronize()
        out.append((ids.cpu().numpy(), state.cpu().numpy(), None if filt is None else filt.cpu().numpy()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and (out[0][0] > 0).sum() > 20
    assert kp is None or np.array_equal(out[0][2], out[1][2])
    assert aw.steps_of(out[1][1], K, M) == [0] * K
    # and the witness under GREEDY says the same
    run_stream(hip, frames, p, kp, M, assign=aw.GREEDY)


@pytest.mark.parametrize("motion", ["none", "kalman"])
def test_a_dense_48_x_48_cluster_is_byte_equal(hip, motion):
    rng = np.random.default_rng(48)
    A, B = aw.dense(rng, 48)
    rows = lambda b, s: np.concatenate([b, s[:, None]], axis=1)
    sc = np.full(48, 0.9)
    frames = [[rows(A, sc)], [rows(B, np.where(np.arange(48) % 5 == 0, 0.3, 0.9))]]
    p, kp = setting(motion, match_thr=0.3, match_thr_low=0.3, min_hits=1)
    (_, got_s, _), tables = run_stream(hip, frames, p, kp, 64, calls=[1, 1])
    steps = aw.steps_of(got_s, 1, 64)[0]
    assert steps > 150, steps      # (far more steps than rows: the searches are long)
    greedy = [tw.new_slot()]
    aw.run(greedy, frames, p, 64, kp, aw.GREEDY)
    assert [t["id"] for t in greedy[0]["tracks"]] != [t["id"] for t in tables[0][0]["tracks"]] or \
        not np.array_equal(tw.state_bytes(greedy, 64, np.zeros(tw.state_layout(1, 64)[3], np.uint8)),
                           tw.state_bytes(tables[0], 64, np.zeros(tw.state_layout(1, 64)[3], np.uint8))), "the walk is optimal here: the case shows nothing"


@pytest.mark.parametrize("motion", ["linear", "kalman"])
def test_three_streams_interleaved_and_one_idle_in_a_call(hip, motion):
    p, kp = setting(motion)
    N = 3
    per = [scene(s, T_=4) for s in (11, 12, 13)]
    for two in (False, True):
        state, filt = fresh(hip, N * K, M, kp is not None)
        other = fresh(hip, N * K, M, kp is not None) if two else (None, None)
        tables = sw.new_tables(N, K)
        frames, so = sw.interleave([f[:2] for f in per], [0, 1, 2, 2, 1, 0])
        acall(hip, frames, so, tables, p, kp, M, state, filt, other[0], other[1])
        if two:
            (state, filt), other = other, (state, filt)
        before = [dict(n=s["n"], frame=s["frame"], steps=s["steps"]) for s in tables[1]]
        assert all(b["n"] > 0 and b["steps"] > 0 for b in before), "the idle stream holds nothing: the case shows nothing"
        frames, so = sw.interleave([per[0][2:], [], per[2][2:]], [2, 0, 0, 2])      # stream 1 has no frame in this call
        acall(hip, frames, so, tables, p, kp, M, state, filt, other[0], other[1])
        assert before == [dict(n=s["n"], frame=s["frame"], steps=s["steps"]) for s in tables[1]]


@pytest.mark.parametrize("motion", ["linear", "kalman"])
def test_the_bounds_a_full_table_of_1024_and_a_sparse_frame_of_1030(hip, motion):
    """Disjoint boxes, each overlapped by one detection: every thread's row and column role at about 1024 searches of one step."""
    m = 1024
    first = tc.crowd(1030, 5)
    second = first.copy()
    second[:, :2] += 0.25                                     # every object moves a little
    second[5:15, 0] += 1000.0                                 # ten of them are gone, ten new ones stand elsewhere
    second[20:40, 4] = 0.3                                    # twenty come through pass 2
    p, kp = setting(motion, min_hits=1, max_age=3, match_thr=0.3, match_thr_low=0.3)
    (_, got_s, _), tables = run_stream(hip, [[first], [second], [second]], p, kp, m, calls=[1, 2])
    s = tables[0][0]
    assert s["n"] == 1024 and s["skipped"] == 18 and s["dropped"] == 20, (s["n"], s["skipped"], s["dropped"])
    assert aw.steps_of(got_s, 1, m) == [s["steps"]] and 2000 <= s["steps"] <= 2048, s["steps"]


def test_guard_bytes_around_the_outputs_are_untouched(hip, scene_facts):
    arena = guarded.Arena("cuda")
    for motion in ("linear", "kalman"):
        p, kp = setting(motion)
        for two in (False, True):
            al = lambda n: arena.alloc(n, torch.uint8)
            state, filt = fresh(hip, K, M, kp is not None, alloc=al)
            other = fresh(hip, K, M, kp is not None, alloc=al) if two else (None, None)
            ids = arena.alloc(T * K * seg_cap_of(scene_facts), torch.int32)
            acall(hip, scene_facts, None, sw.new_tables(1, K), p, kp, M, state, filt, other[0], other[1], ids=ids)
            arena.check()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_names_its_value_and_stores_nothing(hip):
    frames = scene(T_=2)
    buf, offs, cap = tw.pack_bytes(frames, seg_cap_of(frames))
    pack = torch.from_numpy(buf).cuda()
    state, filt = fresh(hip, 2 * K, M, True)
    big = torch.full((state.numel() + filt.numel() + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    ids = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
    s0, f0 = state.clone(), filt.clone()
    lin, kal = setting("linear")[0], setting("kalman")[0]

    def refused(match, p=None, kp=None, kalman=True, **over):
        a = dict(assign="optimal", T=2, K=K, N=1, so=None, pack=pack, cap=cap, si=state, fi=filt if kalman else None, M=M, so_=None, fo_=None, ids=ids)
        a.update(over)
        with pytest.raises(hip.MscnnError, match=match):
            hip.tracks_update_assign(cparams(hip, p or (kal if kalman else lin)), ckparams(hip, (kp or kw.kparams()) if kalman else None), a["assign"],
                                     a["T"], a["K"], a["N"], a["so"], a["pack"], a["cap"], a["si"], a["M"], filter_in=a["fi"], state_out=a["so_"],
                                     filter_out=a["fo_"], ids=a["ids"])
        torch.cuda.synchronize()
        assert torch.equal(state, s0) and torch.equal(filt, f0) and bool((ids == -1).all()) and guarded.all_poison(big), "a refused call stored"

    for kalman in (False, True):
        refused(r"tracks_update_assign: assign 3 is neither 1 \(greedy\) nor 2 \(optimal\)", kalman=kalman, assign=3)
        refused(r"tracks_update_assign: assign 0 is neither", kalman=kalman, assign=0)
        refused(r"tracks_update_assign: num_frames 0", kalman=kalman, T=0)
        refused(r"tracks_update_assign: num_slots 0", kalman=kalman, K=0)
        refused(r"max_tracks 1025 is outside \[1, 1024\]", kalman=kalman, M=1025)
        refused(r"match_thr 1 is not inside", kalman=kalman, p=dict(kal if kalman else lin, match_thr=1.0))
        refused(r"num_streams 257 is outside \[1, 256\]", kalman=kalman, N=257, so=[0, 0])
        refused(r"null stream_of", kalman=kalman, N=2)
        refused(r"stream_of\[1\] = 2 is outside \[0, 2\)", kalman=kalman, N=2, so=[0, 2])
        refused(r"state_out must be 16-byte aligned", kalman=kalman, so_=big[8:8 + state.numel()])
    refused(r"motion 3 is neither 1 \(none\) nor 2 \(linear\)", kalman=False, p=dict(lin, motion=3))
    refused(r"vel_gain 0 is not inside \(0, 1\]", kalman=False, p=dict(lin, vel_gain=0.0))
    refused(r"filter_in is given without a filter", kalman=False, fi=filt)
    refused(r"filter_out is given without a filter", kalman=False, fo_=filt)
    refused(r"motion 2 is not 1 \(none\)", p=dict(kal, motion=2))
    refused(r"std_position nan is not a finite number above 0", kp=dict(kw.kparams(), sp=np.float64("nan")))
    refused(r"filter_out must be 16-byte aligned", fo_=big[8:8 + filt.numel()])
    refused(r"filter_in and filter_out overlap \(\d+ bytes each\) without being equal", fi=big[:filt.numel()], fo_=big[160:160 + filt.numel()])
    # what the wrapper cannot send: a wrong size, null pointers
    L = hip.lib()
    tp, fp = cparams(hip, kal), ckparams(hip, kw.kparams())

    def raw(**over):
        c = hip.TracksAssignCall(C.sizeof(hip.TracksAssignCall), C.addressof(tp), C.addressof(fp), 2, 2, K, 1, None, pack.data_ptr(), cap,
                                 state.data_ptr(), state.data_ptr(), filt.data_ptr(), filt.data_ptr(), M, ids.data_ptr(), hip._stream().value)
        for k, v in over.items():
            setattr(c, k, v)
        assert L.mscnn_tracks_update_assign_fwd(C.byref(c)) != 0
        torch.cuda.synchronize()
        assert torch.equal(state, s0) and torch.equal(filt, f0) and bool((ids == -1).all())
        return L.mscnn_last_error().decode()
    assert f"size {C.sizeof(hip.TracksAssignCall) - 8} is not sizeof(mscnn_tracks_assign_call) = {C.sizeof(hip.TracksAssignCall)}" in \
        raw(size=C.sizeof(hip.TracksAssignCall) - 8)
    for field in ("filter_in", "filter_out"):
        assert raw(**{field: None}).endswith(f"null {field}")
    assert "null pointer" in raw(track=None)
    assert L.mscnn_tracks_update_assign_fwd(None) != 0 and "null call" in L.mscnn_last_error().decode()


# ---- the stream contract -------------------------------------------------------------------------------------------------------------------------
def _stream_case():
    """The gated case of mscnn_tracks_update_assign_fwd (tests/streams.py): six frames of two slots as two streams of three, the optimal
    form under the Kalman filter, on the stream the call struct names."""
    N = 2
    order = [0, 1, 0, 1, 0, 1]
    p, kp = setting("kalman", min_hits=1)
    cache = {}

    def gen(seed):
        if seed not in cache:
            per = [scene(seed, T_=3), scene(seed + 50, T_=3)]
            buf, offs, cap, frames, stream_of = sw.pack_bytes(per, order, 12, "merge")
            cache[seed] = (dict(pack=buf), dict(frames=frames, offs=offs, cap=cap, stream_of=stream_of))
        return cache[seed]

    def run(hip, s, b):
        x = gen(1701)[1]
        state, filt = fresh(hip, N * K, M, True)
        ids = torch.full((x["cap"],), -1, dtype=torch.int32, device="cuda")
        hip.tracks_update_assign(cparams(hip, p), ckparams(hip, kp), "optimal", T, K, N, x["stream_of"], b["pack"], x["cap"], state, M, filter_in=filt,
                                 ids=ids)
        return [ids, state, filt]

    def check(orc, i, o):
        x = gen(1701)[1]
        tables = sw.new_tables(N, K)
        wids = aw.run_streams(tables, x["frames"], x["stream_of"], p, M, kp)
        flat = [slot for tab in tables for slot in tab]
        assert np.array_equal(o[0], want_ids(x["frames"], wids, x["offs"], x["cap"]))
        assert (o[0] > 0).sum() > 10, "nothing was tracked: the case shows nothing"
        assert np.array_equal(o[1], aw.state_bytes(flat, M, np.full(len(o[1]), 0xFF, np.uint8)))
        assert np.array_equal(o[2], kw.filter_bytes(flat, M, np.full(len(o[2]), 0xFF, np.uint8)))

    return streams.Case("tracks_assign", ("mscnn_tracks_state_reset", "mscnn_tracks_update_assign_fwd"), lambda seed: gen(seed)[0], run, check)


def test_gated_the_op_waits_for_nothing_and_runs_in_its_streams_order(hip):
    streams.run_gated(_stream_case(), hip, None, torch.cuda.Stream())


# ---- the Net -------------------------------------------------------------------------------------------------------------------------------------
import test_gpu_seq as gq                        # noqa: E402  (clip_net, small_u8: the small synthetic frames of the Seq-NMS net tests)
import test_gpu_track as gt                      # noqa: E402  (flat_multi, thresholds, frames_of, same_ids, live; the drivers' helpers)
import test_gpu_track_kalman as gk               # noqa: E402  (live_filter)
from mscnn_amd import net as mnet                # noqa: E402


def op_on(hip, frames, p, kp, m, assign, tabs=None, N=1, so=None):
    """The op on the pack of these frames as a batched forward writes it: (ids[t][k], (state, filter))."""
    T_, K_ = len(frames), len(frames[0])
    buf, offs, cap = tw.pack_bytes(frames, seg_cap_of(frames), "image")
    state, filt = fresh(hip, N * K_, m, kp is not None) if tabs is None else tabs
    _, _, ids = hip.tracks_update_assign(cparams(hip, p), ckparams(hip, kp), assign, T_, K_, N, so, torch.from_numpy(buf).cuda(), cap, state, m,
                                         filter_in=filt)
    ids = ids.cpu().numpy()
    return [[ids[offs[t * K_ + k]:offs[t * K_ + k] + len(frames[t][k])] for k in range(K_)] for t in range(T_)], (state, filt)


@pytest.mark.parametrize("kalman", [False, True], ids=["linear", "kalman"])
@pytest.mark.parametrize("N", [1, 2], ids=["one_stream", "two_streams"])
def test_net_optimal_gives_the_ops_bytes_and_greedy_again_what_greedy_gave(hip, kalman, N):
    T_, classes, m = 4, [2, 3], 64
    so = [0, 1, 0, 1] if N == 2 else None
    n, prm, R = gq.clip_net([gq.small_u8(47, 2 * t) for t in range(T_)])
    plain = n.detect_multi(prm, classes)
    with pytest.raises(mnet.NetError, match="set_tracker_assign: the tracker is off"):
        n.set_tracker_assign("optimal")
    hi, lo = gt.thresholds(plain)
    kws = dict(high_thr=hi, low_thr=lo, match_thr=0.2, match_thr_low=0.3, motion="none" if kalman else "linear", max_age=2, min_hits=1, max_tracks=m)
    p, kp = tw.params(**{k: v for k, v in kws.items() if k != "max_tracks"}), (kw.kparams() if kalman else None)
    frames = gt.frames_of(plain)
    K_ = len(frames[0])

    def start():
        n.set_tracker(streams=N, **kws)
        if N > 1:
            n.set_frame_streams(so)
        if kalman:
            n.set_tracker_kalman()

    def tables_are(tabs):
        st = n.tracker_state()
        ns = [s["n"] for tab in (st if N > 1 else [st]) for s in tab]
        assert sum(ns) > 0 and np.array_equal(gt.live(n.tracker_state(raw=True), N * K_, m), gt.live(tabs[0].cpu().numpy(), N * K_, m))
        if kalman:
            assert gk.live_filter(n.tracker_kalman_state(raw=True), ns, m) == gk.live_filter(tabs[1].cpu().numpy(), ns, m)
        return st if N > 1 else [st]

    start()
    assert n.get_tracker_assign() == "greedy"
    assert gt.flat_multi(n.detect_multi(prm, classes)) == gt.flat_multi(plain)
    greedy_ids, greedy_state = n.detect_tracks(), n.tracker_state(raw=True)
    st = n.tracker_state()
    assert all("steps" not in s for tab in (st if N > 1 else [st]) for s in tab), "tracker_state() of a greedy tracker changed"
    # optimal on a fresh table: the op's ids and tables, word 5 included (live() keeps the headers)
    start()
    n.set_tracker_assign("optimal")
    assert n.get_tracker_assign() == "optimal" and (n.get_tracker_kalman() is not None) == kalman and n.get_tracker_streams() == N
    assert gt.flat_multi(n.detect_multi(prm, classes)) == gt.flat_multi(plain), "the assignment changed the detections"
    want, tabs = op_on(hip, frames, p, kp, m, "optimal", N=N, so=so)
    assert gt.same_ids(n.detect_tracks(), want), "the Net's ids are not the op's"
    st = tables_are(tabs)
    steps = hip.tracks_state_steps(tabs[0].cpu().numpy(), N * K_, m)
    assert [s["steps"] for tab in st for s in tab] == steps and sum(steps) > 0
    # switched between calls, the tables untouched: the next call goes on from them under the walk
    n.set_tracker_assign("greedy")
    n.detect_multi(prm, classes)
    want2, tabs = op_on(hip, frames, p, kp, m, "greedy", tabs, N=N, so=so)
    assert gt.same_ids(n.detect_tracks(), want2)
    st = tables_are(tabs)
    assert [s["frame"] for tab in st for s in tab] == [2 * T_ // N] * (N * K_)
    # greedy on a fresh table again: what greedy gave
    n.tracker_reset()
    n.detect_multi(prm, classes)
    assert gt.same_ids(n.detect_tracks(), greedy_ids)
    assert np.array_equal(gt.live(n.tracker_state(raw=True), N * K_, m), gt.live(greedy_state, N * K_, m))
    n.set_tracker(None)
    with pytest.raises(mnet.NetError, match="set_tracker_assign: the tracker is off"):
        n.set_tracker_assign("greedy")


# ---- the drivers ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tool,common", [("run_mscnn_detection.py", ["--cls-ids", "2"]), ("run_cascademscnn.py", gq.CASCADE[:-2])])
def test_driver_track_assign_optimal_leaves_the_result_files_alone_and_writes_tracks(hip, tmp_path, monkeypatch, capsys, tool, common):
    drv = gt.driver(tool, monkeypatch)
    common = gt.common_of(tool, common, tmp_path) + ["--synthetic", "6", "--batch", "2"]
    plain = gt.run_main(drv, tmp_path / "plain", *common)
    called = []
    real = mnet.Net.set_tracker_assign
    monkeypatch.setattr(mnet.Net, "set_tracker_assign", lambda self, *a: (called.append(a), real(self, *a))[1])
    tracks = tmp_path / "tracks"
    tracked = gt.run_main(drv, tmp_path / "tracked", *common, "--track", "--track-high", "0.05", "--track-low", "0.01", "--track-match", "0.2",
                          "--track-assign", "optimal", "--tracks-out", str(tracks))
    capsys.readouterr()
    assert tracked == plain and len(plain) == 1, "--track-assign optimal changed a result file"
    assert called == [("optimal",)]
    name = list(plain)[0].replace("_results", "")
    assert sorted(os.listdir(tracks)) == [name]
    rows = gq.parsed((tracks / name).read_bytes(), 7)
    dets = gq.parsed(plain[list(plain)[0]], 6)
    assert len(dets) > 4 and np.array_equal(rows[:, [0, 2, 3, 4, 5, 6]], dets) and (rows[:, 1] > 0).any()
