"""The tracker's Kalman filter without a GPU: the witness's two restatements against each other (tests/track_kalman_witness.py), the
cases that say when the filter helps and when it does not, the library's exports and struct sizes, and the Net's setting on a
graph-only net."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import track_cases as tc
import track_kalman_witness as kw
import track_witness as tw
from mscnn_amd import hipapi, net as mnet, zoo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_decoupled_filter_is_the_textbook_eight_state_filter():
    """(a), four two-state filters in the header's statements, against (b), F P F^T + Q and P - K S K^T on 8 x 8 matrices: 200 random
    tracks over 40 frames with 30 % misses.  Mean within 1e-9 of max(1, |mean|), covariance entries within 1e-9 of their own size, (b)'s
    cross terms exactly 0.  The bar is a sketch's worst, 2.6e-12, with a 400 x margin; measured here: mean 1.3e-14, covariance 6.4e-14."""
    rng = np.random.default_rng(20221)
    kp = kw.kparams()
    worst_x = worst_p = 0.0
    for _ in range(200):
        b = np.array([rng.uniform(0, 500), rng.uniform(0, 300), rng.uniform(10, 120), rng.uniform(20, 200)])
        vel = rng.uniform(-6, 6, 2)
        grow = rng.uniform(0.97, 1.03)
        fa, fb = kw.birth(b, kp), kw.Textbook(b, kp)
        misses = 0
        for t in range(40):
            b = np.array([b[0] + vel[0], b[1] + vel[1], b[2] * grow, b[3] * grow])
            kw.predict(fa, misses, kp)
            fb.predict(misses)
            if rng.random() < 0.3:
                misses += 1
            else:
                z = b + rng.normal(0, 1.5, 4)
                kw.correct(fa, z, kp)
                fb.correct(z)
                misses = 0
            assert not fb.cross_terms().any(), "the eight-state form's cross terms are not exactly 0"
            mean = np.concatenate([fa["x"], fa["v"]])
            worst_x = max(worst_x, float(np.max(np.abs(mean - fb.x) / np.maximum(1, np.abs(fb.x)))))
            for c in range(4):
                for got, want in ((fa["p"][c], fb.P[c, c]), (fa["q"][c], fb.P[c, c + 4]), (fa["q"][c], fb.P[c + 4, c]), (fa["r"][c], fb.P[c + 4, c + 4])):
                    worst_p = max(worst_p, abs(got - want) / abs(want) if want != 0 else abs(got))
    print(f"decoupled against textbook: worst mean {worst_x:.3g}, worst covariance {worst_p:.3g}")
    assert worst_x < 1e-9 and worst_p < 1e-9, (worst_x, worst_p)


def ids_under(frames, motion, match_thr, kp=None, max_tracks=16, **over):
    """The ids of every frame of a one-slot stream under a motion ("none", "linear", "kalman"), and the slot."""
    p = dict(tw.params(match_thr=match_thr, min_hits=1, motion="none" if motion == "kalman" else motion, **over), motion=motion)
    if motion != "kalman":
        p["motion"] = tw.MOTIONS[motion]
    slot = tw.new_slot()
    return [kw.any_motion(slot, fr[0], p, kp or kw.kparams(), max_tracks).tolist() for fr in frames], slot


def jitter_stream(width=48.0, jitter=6.0):
    """A width x 80 box whose centre moves 10 px a frame with an alternating error of +-jitter, seen in frames 0 .. 9, missed in
    10 .. 12, seen again in 13.  (Width 48 and jitter 6: at 32 and 8 the frame-to-frame overlap of the seen frames falls below 0.3
    under motion none, and the case would show nothing.)"""
    fr = []
    for t in range(14):
        if 10 <= t <= 12:
            fr.append([tc.rows()])
            continue
        cx = 100.0 + 10.0 * t + (jitter if t % 2 == 0 or t == 13 else -jitter)
        fr.append([tc.rows([cx - width / 2, 50.0, width, 80.0, 0.9])])
    return fr


def test_the_filter_keeps_a_jittering_box_over_three_missed_frames_and_the_linear_rule_does_not():
    frames = jitter_stream()
    got = {m: ids_under(frames, m, 0.3)[0] for m in ("none", "linear", "kalman")}
    for m, ids in got.items():      # the preconditions: the case cannot pass empty
        assert ids[:10] == [[1]] * 10 and ids[10:13] == [[]] * 3, (m, ids)
    assert got["kalman"][13] == [1] and got["linear"][13] == [2], got
    _, slot = ids_under(frames[:10], "kalman", 0.3)
    v = slot["tracks"][0]["kf"]["v"][0]
    _, slot = ids_under(frames[:10], "linear", 0.3)
    print(f"velocity after ten seen frames: kalman {v:.3g}, linear {slot['tracks'][0]['vel'][0]:.3g}, true 10")
    assert abs(v - 10) < abs(slot["tracks"][0]["vel"][0] - 10)


def test_on_a_clean_approaching_box_the_linear_rule_keeps_the_id_where_the_filter_loses_it():
    """What the help text says about when not to use the filter: a noise-free box that grows by a fifth per frame and moves with its
    size.  At match_thr 0.4 the linear rule (box snapped to the detection, exact velocity) keeps id 1, the filter (a smoothed size that
    lags) does not; at 0.3 both keep it."""
    frames = []
    for t in range(5):
        s = 1.2 ** t
        w, h = 20 * s, 40 * s
        frames.append([tc.rows([100 + 6 * t * s - w / 2, 100.0 - h / 2, w, h, 0.9])])
    assert ids_under(frames, "linear", 0.4)[0] == [[1]] * 5
    assert ids_under(frames, "kalman", 0.4)[0] != [[1]] * 5
    assert ids_under(frames, "linear", 0.3)[0] == ids_under(frames, "kalman", 0.3)[0] == [[1]] * 5


def test_freeze_lost_height_changes_the_box_over_a_gap_and_nothing_else():
    frames = []
    for t in range(9):
        s = 1.05 ** t
        frames.append([tc.rows() if t in (6, 7) else tc.rows([50.0 + 4 * t, 60.0, 30 * s, 60 * s, 0.9])])
    out = {}
    for freeze in (True, False):
        slot = tw.new_slot()
        boxes = []
        p = tw.params(match_thr=0.3, min_hits=1, motion="none")
        for fr in frames[:8]:
            kw.update(slot, fr[0], p, kw.kparams(freeze_lost_height=freeze), 16)
            boxes.append(slot["tracks"][0]["box"].copy())
        out[freeze] = (boxes, slot)
    for t in range(7):      # up to and including the first missed frame (its prediction still has misses == 0) nothing differs
        assert np.array_equal(out[True][0][t], out[False][0][t]), t
    assert out[True][0][7][3] == out[True][0][6][3] and out[False][0][7][3] > out[False][0][6][3]
    a, b = out[True][1]["tracks"][0], out[False][1]["tracks"][0]
    assert a["id"] == b["id"] and a["hits"] == b["hits"] and a["misses"] == b["misses"] == 2
    for c in range(3):      # centre and aspect do not feel the setting; nor does any covariance
        assert a["kf"]["x"][c] == b["kf"]["x"][c] and a["kf"]["v"][c] == b["kf"]["v"][c]
    for f in ("p", "q", "r"):
        assert np.array_equal(a["kf"][f], b["kf"][f])


def test_a_birth_with_height_0_matches_nothing_and_dies():
    p = tw.params(match_thr=0.3, min_hits=1, max_age=2, motion="none")
    slot = tw.new_slot()
    flat = tc.rows([10.0, 10.0, 20.0, 0.0, 0.9])
    assert kw.update(slot, flat, p, kw.kparams(), 16).tolist() == [1]
    assert np.isinf(slot["tracks"][0]["kf"]["x"][2])
    ids = [kw.update(slot, flat, p, kw.kparams(), 16).tolist() for _ in range(3)]
    assert ids == [[2], [3], [4]], ids      # every frame's flat box starts a track of its own: it pairs with nothing
    assert not np.isfinite(slot["tracks"][0]["box"]).all()
    assert [t["id"] for t in slot["tracks"]] == [2, 3, 4], "track 1 has not aged out after max_age missed frames"


def test_filter_bytes_and_attach_filter_are_inverse():
    frames = tc.drift_stream(3, T=6, K=2)
    p = tw.params(high_thr=0.5, low_thr=0.125, match_thr=0.1, match_thr_low=0.25, motion="none", max_age=2, min_hits=2)
    slots = [tw.new_slot(), tw.new_slot()]
    kw.run(slots, frames, p, kw.kparams(), 16)
    assert sum(s["n"] for s in slots) > 4
    sb = tw.state_bytes(slots, 16, np.full(tw.state_layout(2, 16)[3], 0xFF, np.uint8))
    fb = kw.filter_bytes(slots, 16, np.full(2 * 16 * kw.RECORD_BYTES, 0xFF, np.uint8))
    back = kw.attach_filter(tw.parse_state(sb, 2, 16), fb, 16)
    assert np.array_equal(kw.filter_bytes(back, 16, np.full(fb.size, 0xFF, np.uint8)), fb)
    assert np.array_equal(tw.state_bytes(back, 16, np.full(sb.size, 0xFF, np.uint8)), sb)


# ---- the library and the Net ---------------------------------------------------------------------------------------------------------------------
def test_exports_and_struct_sizes(tmp_path):
    L = hipapi.lib()
    assert hasattr(L, "mscnn_tracks_update_kalman_fwd") and hasattr(L, "mscnn_tracks_kalman_state_bytes")
    for name in ("mscnn_net_set_tracker_kalman", "mscnn_net_get_tracker_kalman", "mscnn_net_tracker_kalman_state"):
        assert hasattr(mnet.lib(), name), name
    assert hipapi.TRACK_KALMAN_RECORD.itemsize == mnet.TRACK_KALMAN_RECORD.itemsize == kw.RECORD_BYTES == 160
    assert hipapi.tracks_kalman_state_bytes(6, 16) == 6 * 16 * 160 and hipapi.tracks_kalman_state_bytes(6, 1025) == 0
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mscnn_net.h"\n#include "mscnn_hip.h"\n#include "mscnn_net.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(mscnn_track_kalman_record), sizeof(mscnn_track_kalman_params), '
                   'sizeof(mscnn_tracks_kalman_call), offsetof(mscnn_tracks_kalman_call, stream), sizeof(mscnn_track_record)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [160, C.sizeof(hipapi.TrackKalmanParams), C.sizeof(hipapi.TracksKalmanCall), hipapi.TracksKalmanCall.stream.offset, 104], got
    assert C.sizeof(hipapi.TrackKalmanParams) == C.sizeof(mnet.TrackKalmanParams) == 48


def test_the_header_says_why_the_op_takes_one_argument_and_what_a_flat_birth_does():
    text = " ".join(open(os.path.join(ROOT, "include", "mscnn_hip.h")).read().split())
    assert "ONE argument: the op would have 17" in text
    assert "A birth with h <= 0 gets a NaN / inf" in text
    assert re.search(r"tracks_update_kalman_fwd\s+pack_dev, state_in, state_out, filter_in, filter_out 16, track_ids_dev 4: refuses", text)


def graph_net():
    return mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=96, width=320), device=-1)


def test_net_set_get_and_refusals_without_a_device():
    n = graph_net()
    assert n.get_tracker_kalman() is None
    with pytest.raises(mnet.NetError, match="set_tracker_kalman: the tracker is off"):
        n.set_tracker_kalman()
    n.set_tracker_kalman(None)                                     # off while off: nothing happens
    n.set_tracker(motion="linear")
    with pytest.raises(mnet.NetError, match=r"set_tracker_kalman: the tracker's motion 2 is not 1 \(none\)"):
        n.set_tracker_kalman()
    assert n.get_tracker_kalman() is None
    n.set_tracker(motion="none", streams=3)
    n.set_frame_streams([0, 2, 1])
    n.set_tracker_kalman(std_position=0.1, freeze_lost_height=False)
    want = dict(std_position=0.1, std_velocity=1 / 160, std_aspect=1e-2, std_aspect_velocity=1e-5, std_aspect_measure=1e-1, freeze_lost_height=False)
    assert n.get_tracker_kalman() == want
    assert n.get_tracker_streams() == 3 and n.get_frame_streams() == [0, 2, 1], "the filter's setting moved the streams or the mapping"
    for field in ("std_position", "std_velocity", "std_aspect", "std_aspect_velocity", "std_aspect_measure"):
        for bad in (float("nan"), float("inf"), 0.0, -1.0):
            with pytest.raises(mnet.NetError, match=f"set_tracker_kalman: {field} .* is not a finite number above 0"):
                n.set_tracker_kalman(**{field: bad})
            assert n.get_tracker_kalman() == want, "a refused value changed the setting"
    with pytest.raises(mnet.NetError, match="tracker_kalman_state: no tracked call has succeeded"):
        n.tracker_kalman_state()
    n.set_tracker_kalman(None)
    assert n.get_tracker_kalman() is None and n.get_tracker()["motion"] == "none" and n.get_tracker_streams() == 3
    n.set_tracker_kalman()
    n.set_tracker(motion="none")                                   # set_tracker turns the filter off, as it puts the streams back to 1
    assert n.get_tracker_kalman() is None and n.get_tracker_streams() == 1
    with pytest.raises(mnet.NetError, match="motion 'kalman' is none of"):
        n.set_tracker(motion="kalman")
    with pytest.raises(mnet.NetError, match="tracker_kalman_state: the filter is off"):
        n.tracker_kalman_state()


@pytest.mark.parametrize("tool", ["run_mscnn_detection.py", "run_cascademscnn.py"])
def test_the_drivers_refuse_the_filter_flags_without_their_owner(tool):
    import sys
    exe = [sys.executable, os.path.join(ROOT, "tools", tool), "--synthetic", "1"]
    r = subprocess.run(exe + ["--track-kalman-pos", "0.1"], capture_output=True, text=True)
    assert r.returncode == 2 and "belong to --track" in r.stderr, r.stderr[-400:]
    r = subprocess.run(exe + ["--track", "--track-kalman-vel", "0.1"], capture_output=True, text=True)
    assert r.returncode == 2 and "belong to --track-motion kalman" in r.stderr, r.stderr[-400:]
    r = subprocess.run(exe + ["--track-motion", "kalman"], capture_output=True, text=True)
    assert r.returncode == 2 and "belong to --track" in r.stderr, r.stderr[-400:]
