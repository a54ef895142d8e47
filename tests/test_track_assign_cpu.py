"""The tracker's optimal assignment without a GPU: the witness (tests/track_assign_witness.py) against an exhaustive search and
scipy, the greedy walk against the optimum, the four-box example where the walk loses a track, the step bound, the case where both
forms agree, the library's exports and struct size, the Net's setting on a graph-only net, the drivers' flag."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import track_assign_witness as aw
import track_kalman_witness as kw
import track_witness as tw
from mscnn_amd import hipapi, net as mnet, zoo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, CASES, THR = 1, 300, 0.3


@pytest.fixture(scope="module")
def cases():
    """300 seeded clusters of at most 6 x 6 boxes (centres sigma 6 px around three points, sizes 20 .. 30 px): (r, a, b), made once."""
    rng = np.random.default_rng(SEED)
    out = []
    for _ in range(CASES):
        a, b = (int(v) for v in rng.integers(1, 7, size=2))
        A, B = aw.cluster(rng, a, b)
        out.append((tw.overlap_pairs(A, B), a, b))
    return out


def test_the_matching_is_a_maximum_weight_matching(cases):
    """The total weight equals an exhaustive search on every case; every matched pair is eligible, nothing is matched twice."""
    matched = 0
    for r, a, b in cases:
        pairs, _ = aw.match_optimal(r, THR, list(range(a)), list(range(b)))
        assert aw.total_weight(r, THR, pairs) == aw.brute_force(r, THR, range(a), range(b))
        assert len(set(pairs.values())) == len(pairs) and all(0 <= i < a and 0 <= j < b for i, j in pairs.items())
        assert all(r[i, j] > THR for i, j in pairs.items()), "a matched pair is not eligible"
        matched += len(pairs)
    assert matched > CASES, "hardly anything was matched: the cases show nothing"


def test_the_matching_is_scipys_linear_sum_assignment(cases):
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    for r, a, b in cases:
        W = np.zeros((a, b), np.int64)      # an absent pair weighs 0: taking it is leaving both ends unmatched
        for (i, j), w in aw.weights(r, THR, range(a), range(b)).items():
            W[i, j] = w
        ri, ci = lsa(W, maximize=True)
        pairs, _ = aw.match_optimal(r, THR, list(range(a)), list(range(b)))
        assert aw.total_weight(r, THR, pairs) == int(W[ri, ci].sum())


def test_dense_clusters_match_scipy_and_keep_the_step_bound():
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    for n in (8, 16, 32, 48, 64):
        A, B = aw.dense(np.random.default_rng(n), n)
        r = tw.overlap_pairs(A, B)
        pairs, steps = aw.match_optimal(r, THR, list(range(n)), list(range(n)))
        W = np.zeros((n, n), np.int64)
        for (i, j), w in aw.weights(r, THR, range(n), range(n)).items():
            W[i, j] = w
        ri, ci = lsa(W, maximize=True)
        assert aw.total_weight(r, THR, pairs) == int(W[ri, ci].sum())
        greedy, _ = tw.match_walk(r, THR, list(range(n)), list(range(n)))
        assert aw.total_weight(r, THR, greedy) < aw.total_weight(r, THR, pairs), "the walk is optimal on a dense cluster?"
        assert n < steps <= n * (n + 1)


def test_the_greedy_walk_is_never_above_and_sometimes_below_the_optimum(cases):
    below = 0
    for r, a, b in cases:
        tr, de = list(range(a)), list(range(b))
        g = aw.total_weight(r, THR, tw.match_walk(r, THR, tr, de)[0])
        o = aw.total_weight(r, THR, aw.match_optimal(r, THR, tr, de)[0])
        assert g <= o
        below += g < o
    assert below == 11, below      # (the generator under SEED)


def test_steps_keep_their_bound_and_rows_without_a_pair_cost_none(cases):
    for r, a, b in cases:
        _, steps = aw.match_optimal(r, THR, list(range(a)), list(range(b)))
        with np.errstate(invalid="ignore"):
            rows = int((r > THR).any(axis=1).sum())
        assert rows <= steps <= rows * (min(a, b) + 1) <= a * (min(a, b) + 1)
        if rows == 0:
            assert steps == 0
    # two tracks far from every detection beside one that overlaps: one search of one step
    r = tw.overlap_pairs([[0, 0, 10, 10], [500, 500, 10, 10], [900, 0, 10, 10]], [[1, 0, 10, 10], [300, 300, 10, 10]])
    assert aw.match_optimal(r, THR, [0, 1, 2], [0, 1]) == ({0: 0}, 1)
    assert aw.match_optimal(r, THR, [1, 2], [0, 1]) == ({}, 0) and aw.match_optimal(r, THR, [], [0]) == ({}, 0)


# ---- the four-box example: r(A, b) = 0.65, r(A, a) = 0.60, r(B, b) = 0.50, r(B, a) below the threshold
def box(x):
    return [x, 0.0, 10.0, 10.0, 0.9]


def four_boxes():
    """Boxes of one size on a line; two boxes d apart overlap by (10 - d) / (10 + d).  Frame 1: A at 0, B; frame 2 and 3: a left of
    A, b between A and B."""
    d = lambda r: 10.0 * (1.0 - r) / (1.0 + r)
    xa, xb = -d(0.60), d(0.65)
    xB = xb + d(0.50)
    return [[np.array([box(0.0), box(xB)])], [np.array([box(xa), box(xb)])], [np.array([box(xa), box(xb)])]]


@pytest.mark.parametrize("motion", ["none", "linear", "kalman"])
def test_four_boxes_the_walk_loses_a_track_the_assignment_keeps_both(motion):
    frames = four_boxes()
    r = tw.overlap_pairs(frames[0][0][:, :4], frames[1][0][:, :4])
    assert r[0, 1] > r[0, 0] > r[1, 1] > THR and not r[1, 0] > THR and r[0, 0] + r[1, 1] > r[0, 1]
    kp = kw.kparams() if motion == "kalman" else None
    p = tw.params(match_thr=THR, min_hits=1, motion="none" if motion == "kalman" else motion)
    got = {}
    for assign in (aw.GREEDY, aw.OPTIMAL):
        slot = tw.new_slot()
        got[assign] = [aw.update(slot, fr[0], p, 16, kp, assign).tolist() for fr in frames], slot
    ids, slot = got[aw.GREEDY]
    assert ids[0] == [1, 2] and ids[1] == [3, 1], ids                      # A took b; a starts id 3, B has nothing
    assert 2 not in ids[2] and slot.get("steps", 0) == 0
    ids, slot = got[aw.OPTIMAL]
    assert ids == [[1, 2]] * 3, ids
    assert slot["next_id"] == 3 and slot["steps"] >= 4


def disjoint_stream(T=5, n=9):
    """n objects on a grid 60 px apart, 20 px boxes that jitter by at most 2 px: every track overlaps one detection.  Every third
    object's score drops under high_thr in odd frames, so pass 2 has work."""
    rng = np.random.default_rng(5)
    frames = []
    for t in range(T):
        rows = []
        for o in range(n):
            x, y = 60.0 * (o % 3) + rng.uniform(-2, 2), 60.0 * (o // 3) + rng.uniform(-2, 2)
            rows.append([x, y, 20.0, 20.0, 0.3 if (o % 3 == 0 and t % 2 == 1) else 0.9])
        frames.append([np.array(rows)])
    return frames


@pytest.mark.parametrize("motion", ["none", "linear", "kalman"])
def test_disjoint_boxes_both_forms_give_the_same_ids_and_state_apart_from_word_5(motion):
    frames = disjoint_stream()
    kp = kw.kparams() if motion == "kalman" else None
    p = tw.params(match_thr=THR, match_thr_low=0.3, min_hits=1, motion="none" if motion == "kalman" else motion)
    out = {}
    for assign in (aw.GREEDY, aw.OPTIMAL):
        slots = [tw.new_slot()]
        ids = aw.run(slots, frames, p, 16, kp, assign)
        base = np.full(tw.state_layout(1, 16)[3], 0xFF, np.uint8)
        out[assign] = [i[0].tolist() for i in ids], aw.state_bytes(slots, 16, base, assign), slots
    assert out[aw.GREEDY][0] == out[aw.OPTIMAL][0] == [list(range(1, 10))] * len(frames)
    g, o = out[aw.GREEDY][1].copy(), out[aw.OPTIMAL][1].copy()
    assert g[:32].view(np.int32)[aw.STEPS_WORD] == 0 and o[:32].view(np.int32)[aw.STEPS_WORD] == 9 * (len(frames) - 1)
    g[:32].view(np.int32)[aw.STEPS_WORD] = o[:32].view(np.int32)[aw.STEPS_WORD] = 0
    assert np.array_equal(g, o)
    if kp is not None:
        fb = np.full(16 * kw.RECORD_BYTES, 0xFF, np.uint8)
        assert np.array_equal(kw.filter_bytes(out[aw.GREEDY][2], 16, fb), kw.filter_bytes(out[aw.OPTIMAL][2], 16, fb))
    # the witness's buffers are inverse pairs, word 5 included; the count saturates
    back = aw.parse_state(out[aw.OPTIMAL][1], 1, 16)
    assert back[0]["steps"] == 9 * (len(frames) - 1) == aw.steps_of(out[aw.OPTIMAL][1], 1, 16)[0]
    s = dict(steps=aw.INT32_MAX - 1)
    aw.add_steps(s, 5)
    assert s["steps"] == aw.INT32_MAX


# ---- the library, the Net, the drivers -----------------------------------------------------------------------------------------------------------
def test_exports_and_struct_sizes(tmp_path):
    assert hasattr(hipapi.lib(), "mscnn_tracks_update_assign_fwd")
    for name in ("mscnn_net_set_tracker_assign", "mscnn_net_get_tracker_assign"):
        assert hasattr(mnet.lib(), name), name
    assert hipapi.TRACK_ASSIGNS == dict(greedy=aw.GREEDY, optimal=aw.OPTIMAL) and hipapi.TRACKS_STEPS == aw.STEPS_WORD
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mscnn_net.h"\n#include "mscnn_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %d %d %d %zu\\n", sizeof(mscnn_tracks_assign_call), '
                   'offsetof(mscnn_tracks_assign_call, assign), offsetof(mscnn_tracks_assign_call, filter_in), '
                   'offsetof(mscnn_tracks_assign_call, stream), MSCNN_TRACKS_STEPS, MSCNN_TRACK_ASSIGN_GREEDY, MSCNN_TRACK_ASSIGN_OPTIMAL, '
                   'sizeof(mscnn_tracks_kalman_call)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    call = hipapi.TracksAssignCall
    assert got == [C.sizeof(call), call.assign.offset, call.filter_in.offset, call.stream.offset, 5, 1, 2, C.sizeof(hipapi.TracksKalmanCall)], got


def test_the_header_states_the_second_form_and_no_longer_calls_the_walk_the_only_matching():
    for name in ("include/mscnn_hip.h", "README.md"):
        text = " ".join(open(os.path.join(ROOT, name)).read().split())
        assert "in place of the Hungarian solver" not in text, name
        assert "NOT evaluated" in text or "not evaluated" in text, name
    text = " ".join(open(os.path.join(ROOT, "include", "mscnn_hip.h")).read().split())
    assert "4''." in text and "5''." in text and "MSCNN_TRACKS_STEPS" in text
    assert "tracks_update_assign_fwd" in text


def graph_net():
    return mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=96, width=320), device=-1)


def test_net_set_get_and_refusals_without_a_device():
    n = graph_net()
    assert n.get_tracker_assign() is None
    with pytest.raises(mnet.NetError, match="set_tracker_assign: the tracker is off"):
        n.set_tracker_assign("optimal")
    n.set_tracker(motion="none", streams=2)
    assert n.get_tracker_assign() == "greedy"
    n.set_tracker_kalman()
    n.set_tracker_assign("optimal")
    assert n.get_tracker_assign() == "optimal" and n.get_tracker_kalman() is not None and n.get_tracker_streams() == 2
    with pytest.raises(mnet.NetError, match="assign 'hungarian' is none of"):
        n.set_tracker_assign("hungarian")
    with pytest.raises(mnet.NetError, match=r"set_tracker_assign: assign 3 is neither 1 \(greedy\) nor 2 \(optimal\)"):
        n.set_tracker_assign(3)
    assert n.get_tracker_assign() == "optimal", "a refused value changed the setting"
    n.set_tracker_assign("greedy")
    assert n.get_tracker_assign() == "greedy"
    n.set_tracker_assign("optimal")
    n.set_tracker(motion="linear")                                  # set_tracker puts the matching back to greedy, as it does the streams
    assert n.get_tracker_assign() == "greedy"
    n.set_tracker(None)
    assert n.get_tracker_assign() is None


@pytest.mark.parametrize("tool", ["run_mscnn_detection.py", "run_cascademscnn.py"])
def test_the_drivers_refuse_track_assign_without_track(tool):
    exe = [sys.executable, os.path.join(ROOT, "tools", tool), "--synthetic", "1"]
    r = subprocess.run(exe + ["--track-assign", "optimal"], capture_output=True, text=True)
    assert r.returncode == 2 and "belong to --track" in r.stderr, r.stderr[-400:]
    r = subprocess.run(exe + ["--track", "--track-assign", "hungarian"], capture_output=True, text=True)
    assert r.returncode == 2 and "invalid choice" in r.stderr, r.stderr[-400:]
