"""The tracker for a batch of streams without a GPU: the Net-level settings (mscnn_net_set_tracker_streams, _set_frame_streams,
_get_tracker_streams, _tracker_reset_stream) on a graph-only net -- sticky, round trip, every refusal names its value and leaves the
setting as it was --, and the witness's helpers (tests/track_streams_witness.py): the interleaved pack and state builders invert their
parsers, and the split witness is track_witness run per stream."""
import copy
import ctypes as C
import re

import numpy as np
import pytest

import track_cases as tc
import track_streams_witness as sw
import track_witness as tw
from mscnn_amd import net as mnet, zoo


def graph_net():
    return mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=96, width=320), device=-1)


def test_the_libraries_export_the_stream_ops_and_calls():
    from mscnn_amd import hipapi
    L = hipapi.lib()
    assert hasattr(L, "mscnn_tracks_update_streams_fwd") and hasattr(L, "mscnn_tracks_state_reset_slots")
    assert callable(hipapi.tracks_update_streams) and callable(hipapi.tracks_state_reset_slots)
    N = mnet.lib()
    for name in ("mscnn_net_set_tracker_streams", "mscnn_net_set_frame_streams", "mscnn_net_get_tracker_streams", "mscnn_net_tracker_reset_stream"):
        assert hasattr(N, name), name


def test_net_streams_are_one_by_default_sticky_and_put_back_by_set_tracker():
    n = graph_net()
    assert n.get_tracker_streams() == 1 and n.get_frame_streams() is None
    n.set_tracker(high_thr=0.6, low_thr=0.2, max_tracks=32, streams=3)
    assert n.get_tracker_streams() == 3 and n.get_frame_streams() is None
    assert n.get_tracker() == dict(high_thr=0.6, low_thr=0.2, new_thr=0.6, match_thr=0.3, match_thr_low=0.5, motion="linear", vel_gain=0.5,
                                   max_age=30, min_hits=1, max_tracks=32)
    n.set_frame_streams([2, 0, 0, 1])
    assert n.get_frame_streams() == [2, 0, 0, 1]
    n.set_nms(type="max")                                    # (other sticky settings do not touch these)
    n.set_box_voting(0.4)
    assert n.get_tracker_streams() == 3 and n.get_frame_streams() == [2, 0, 0, 1]
    n.set_frame_streams(None)
    assert n.get_frame_streams() is None and n.get_tracker_streams() == 3
    n.set_frame_streams([1])
    n.set_frame_streams([])
    assert n.get_frame_streams() is None
    n.set_frame_streams(list(range(3)) * 85 + [0])           # 256 entries: the bound
    assert len(n.get_frame_streams()) == 256
    n.tracker_reset(stream=2)                                # K is not fixed yet: succeeds, does nothing
    n.tracker_reset()
    assert n.get_tracker_streams() == 3 and len(n.get_frame_streams()) == 256, "tracker_reset starts the tables again, not the settings"
    # a new set_tracker_streams clears the mapping; set_tracker puts the streams back to 1
    assert mnet.lib().mscnn_net_set_tracker_streams(n._h, 2) == 0
    assert n.get_tracker_streams() == 2 and n.get_frame_streams() is None
    n.set_frame_streams([1, 0])
    n.set_tracker(high_thr=0.6, low_thr=0.2, max_tracks=32)
    assert n.get_tracker_streams() == 1 and n.get_frame_streams() is None
    n.set_tracker(high_thr=0.5, streams=256)
    assert n.get_tracker_streams() == 256
    n.set_tracker(None)
    assert n.get_tracker_streams() == 1 and n.get_tracker() is None


def test_net_stream_refusals_name_the_value_and_leave_the_setting_as_it_was():
    n = graph_net()
    lib = mnet.lib()
    for call_, text in ((lambda: n.set_tracker(None) or mnet._check(lib.mscnn_net_set_tracker_streams(n._h, 2)), "set_tracker_streams: the tracker is off"),
                        (lambda: n.set_frame_streams([0]), "set_frame_streams: the tracker is off"),
                        (lambda: n.tracker_reset(stream=0), "tracker_reset_stream: the tracker is off")):
        with pytest.raises(mnet.NetError, match=text):
            call_()
    assert n.get_tracker() is None and n.get_tracker_streams() == 1
    n.set_frame_streams(None)                                # (clearing needs no tracker)
    with pytest.raises(mnet.NetError, match=r"set_tracker_streams: num_streams 257 is outside \[1, 256\]"):
        n.set_tracker(high_thr=0.5, streams=257)
    assert n.get_tracker() is None, "a refused streams value turned the tracker on"
    kw = dict(high_thr=0.6, low_thr=0.2, max_tracks=32)
    n.set_tracker(**kw, streams=3)
    n.set_frame_streams([0, 2, 1])
    want = n.get_tracker()
    for bad in (0, -1, 257):
        with pytest.raises(mnet.NetError, match=re.escape(f"set_tracker_streams: num_streams {bad} is outside [1, 256]")):
            n.set_tracker(**kw, streams=bad)
        assert (n.get_tracker(), n.get_tracker_streams(), n.get_frame_streams()) == (want, 3, [0, 2, 1]), bad
        assert lib.mscnn_net_set_tracker_streams(n._h, bad) != 0
        assert (n.get_tracker_streams(), n.get_frame_streams()) == (3, [0, 2, 1]), bad
    for bad, text in (([0, 3, 1], "stream_of[1] = 3 is outside [0, 3)"), ([-1], "stream_of[0] = -1 is outside [0, 3)"),
                      ([0] * 257, "count 257 is outside [0, 256]")):
        with pytest.raises(mnet.NetError, match="set_frame_streams: " + re.escape(text)):
            n.set_frame_streams(bad)
        assert n.get_frame_streams() == [0, 2, 1]
    for bad in (-1, 3):
        with pytest.raises(mnet.NetError, match=re.escape(f"tracker_reset_stream: stream {bad} is outside [0, 3)")):
            n.tracker_reset(stream=bad)
    # the getter: a buffer too small for the mapping is refused, naming both numbers
    ns, cnt, so = C.c_int(), C.c_int(), (C.c_int * 2)()
    assert lib.mscnn_net_get_tracker_streams(n._h, C.byref(ns), so, 2, C.byref(cnt)) != 0
    assert "get_tracker_streams: the buffer holds 2 entries, the mapping has 3" in lib.mscnn_net_last_error().decode()
    assert lib.mscnn_net_get_tracker_streams(n._h, None, so, 2, C.byref(cnt)) != 0
    # Seq-NMS is one stream: refused in both directions, naming the setting
    with pytest.raises(mnet.NetError, match=r"set_seq_nms: link_thr 0.5 while the tracker has 3 streams \(set_tracker_streams\)"):
        n.set_seq_nms(0.5)
    assert n.get_seq_nms() is None and n.get_tracker_streams() == 3
    n.set_tracker(**kw)
    n.set_seq_nms(0.5)                                       # (one stream: the two go together as before)
    with pytest.raises(mnet.NetError, match=r"set_tracker_streams: num_streams 2 while Seq-NMS is on \(set_seq_nms link_thr 0.5\)"):
        n.set_tracker(**kw, streams=2)
    assert n.get_tracker_streams() == 1 and n.get_tracker() == want and n.get_seq_nms()["link_thr"] == 0.5
    assert lib.mscnn_net_set_tracker_streams(n._h, 1) == 0   # (1 is what it is)


# ---- the witness's helpers ----------------------------------------------------------------------------------------------------------------------
ORDER = [2, 0, 2, 2, 0, 2, 0]                                # three streams with 3, 0 and 4 frames, out of round-robin order


def three_streams(K=2):
    return [tc.drift_stream(21, T=3, K=K), [], tc.grid_stream(22, T=4, K=K)]


def same_frames(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all((u is None and v is None) or np.array_equal(u, v) for u, v in zip(x, y))
                                    for x, y in zip(a, b))


@pytest.mark.parametrize("form", ["merge", "image"])
def test_interleave_split_and_the_pack_builder_invert_each_other(form):
    per = three_streams()
    per[2][1][0] = None                                      # an overflowed segment travels too
    frames, stream_of = sw.interleave(per, ORDER)
    assert stream_of == ORDER and len(frames) == 7
    back, where = sw.split(frames, stream_of, 3)
    assert where == [[1, 4, 6], [], [0, 2, 3, 5]]
    assert all(same_frames(a, b) for a, b in zip(back, per))
    buf, offs, cap, fr2, so2 = sw.pack_bytes(per, ORDER, 14, form)
    assert so2 == ORDER and same_frames(fr2, frames)
    assert same_frames(sw.parse_pack(buf, 7, 2), frames)
    again, _, _ = tw.pack_bytes(sw.parse_pack(buf, 7, 2), 14, form)
    assert np.array_equal(again, buf)
    with pytest.raises(AssertionError):
        sw.interleave(per, ORDER[:-1])


def test_the_state_builder_inverts_its_parser_and_the_split_witness_is_the_witness_per_stream():
    per = three_streams()
    frames, stream_of = sw.interleave(per, ORDER)
    p = tw.params(high_thr=0.5, low_thr=0.125, match_thr=0.1, match_thr_low=0.25, max_age=2)
    tables = sw.new_tables(3, 2)
    ids = sw.run(tables, frames, stream_of, p, 16)
    base = np.full(tw.state_layout(6, 16)[3], 0xFF, np.uint8)
    b = sw.state_bytes(tables, 16, base)
    again = sw.state_bytes(sw.parse_state(b, 3, 2, 16), 16, base)
    assert np.array_equal(b, again)
    fresh = tw.state_bytes([tw.new_slot(), tw.new_slot()], 16, np.full(tw.state_layout(2, 16)[2] * 2, 0xFF, np.uint8)[:tw.state_layout(2, 16)[3]])
    assert np.array_equal(sw.block(b, 1, 2, 16), fresh[:len(sw.block(b, 1, 2, 16))]), "the stream without a frame is a fresh table: frame 0, id 1"
    for s in (0, 2):
        alone, want = tc.witness(per[s], p, 16)
        one = tw.state_bytes(alone, 16, np.full(tw.state_layout(2, 16)[3], 0xFF, np.uint8))
        blk = sw.block(b, s, 2, 16)
        assert np.array_equal(blk, one[:len(blk)])
        got = [ids[t] for t in sw.split(frames, stream_of, 3)[1][s]]
        assert all(np.array_equal(x, y) for fa, fb in zip(got, want) for x, y in zip(fa, fb))
        assert [x["frame"] for x in tables[s]] == [len(per[s])] * 2 and tables[s][0]["next_id"] > 3
    # the calls compose: the same per-stream order in another interleaving, cut into two calls, leaves the same tables
    t2 = sw.new_tables(3, 2)
    f_a, so_a = sw.interleave([per[0][:1], [], per[2][:3]], [0, 2, 2, 2])
    f_b, so_b = sw.interleave([per[0][1:], [], per[2][3:]], [2, 0, 0])
    sw.run(t2, f_a, so_a, p, 16)
    keep = copy.deepcopy(t2)
    sw.run(t2, f_b, so_b, p, 16)
    assert np.array_equal(sw.state_bytes(t2, 16, base), b) and not np.array_equal(sw.state_bytes(keep, 16, base), b)
