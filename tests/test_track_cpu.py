"""The tracker's witness on the CPU (tests/track_witness.py, the restatement mscnn_tracks_update_fwd is held to bit for bit): the
literal walk over the sorted pairs and the rounds of mutually-best pairs give the same matching on tables full of exactly equal
overlaps, the facts hold, and hand-worked streams come out as worked by hand."""
import copy

import numpy as np
import pytest

import track_cases as tc
import track_witness as tw


def table(seed, n, m, side):
    rng = np.random.default_rng(seed)
    return tw.overlap_pairs(tc.grid_rows(rng, n, side=side)[:, :4], tc.grid_rows(rng, m, side=side)[:, :4])


@pytest.mark.parametrize("side", [4, 12])
def test_walk_and_rounds_agree_on_tables_with_many_equal_overlaps(side):
    most, ties, matched = 0, 0, 0
    for seed in range(60):
        rng = np.random.default_rng(1000 + seed)
        n, m = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        r = table(seed, n, m, side)
        vals = r[~np.isnan(r)]
        ties += len(vals) - len(np.unique(vals))
        tracks = [i for i in range(n) if rng.random() < 0.8]
        dets = [j for j in range(m) if rng.random() < 0.8]
        for thr in (0.0, 0.1, 0.3, 0.5):
            a, _ = tw.match_walk(r, thr, tracks, dets)
            b, rounds = tw.match_rounds(r, thr, tracks, dets)
            assert a == b, (seed, thr)
            assert rounds <= min(len(tracks), len(dets))
            most = max(most, rounds)
            matched += len(a)
    assert ties > 1000 and matched > 500, "no ties, or nothing matched: the case shows nothing"
    assert most >= 2, "one round always: the case shows nothing"


def test_a_stream_is_the_same_under_both_matchings_and_the_facts_hold():
    p = tw.params(high_thr=0.5, low_thr=0.125, match_thr=0.1, match_thr_low=0.25, max_age=2, min_hits=2)
    for seed in range(8):
        frames = tc.drift_stream(seed, T=8, K=2)
        a, ia = tc.witness(frames, p, 16)
        b, ib = tc.witness(frames, p, 16, match=tw.match_rounds)
        base = np.zeros(tw.state_layout(2, 16)[3], np.uint8)
        assert np.array_equal(tw.state_bytes(a, 16, base), tw.state_bytes(b, 16, base))
        assert all(np.array_equal(x, y) for fa, fb in zip(ia, ib) for x, y in zip(fa, fb))
        assert tw.facts([tw.new_slot(), tw.new_slot()], frames, p, 16) >= 1
        assert max(s["next_id"] for s in a) > 5 and any(i.max(initial=0) > 0 for f in ia for i in f)
    # and a table that overflows: births are dropped, n stays at max_tracks
    frames = tc.grid_stream(3, T=4, K=1, counts=(10, 14))
    s, _ = tc.witness(frames, tw.params(high_thr=0.25, low_thr=0.25), 4)
    assert s[0]["n"] == 4 and s[0]["dropped"] > 0
    tw.facts([tw.new_slot()], frames, tw.params(high_thr=0.25, low_thr=0.25), 4)


def test_state_bytes_and_parse_state_are_inverse():
    frames = tc.drift_stream(5, T=5, K=3)
    p = tw.params(match_thr=0.1)
    s, _ = tc.witness(frames, p, 32)
    base = np.full(tw.state_layout(3, 32)[3], 0xFF, np.uint8)
    b = tw.state_bytes(s, 32, base)
    again = tw.state_bytes(tw.parse_state(b, 3, 32), 32, base)
    assert np.array_equal(b, again)
    rec_at, rec, slot, total = tw.state_layout(3, 32)
    assert (rec_at, rec, slot) == (32, 104, 32 + 32 * 104) and total % 16 == 0
    k = 1
    tail = b[k * slot + rec_at + s[k]["n"] * rec:(k + 1) * slot]
    assert len(tail) and (tail == 0xFF).all(), "records at index >= n are left as they were"


def ids_of(frames, p, max_tracks=8):
    s, ids = tc.witness(frames, p, max_tracks)
    return s, [[i.tolist() for i in fr] for fr in ids]


def test_a_low_score_frame_keeps_its_id_through_pass_2_only():
    frames = tc.still([0.9, 0.9, 0.2, 0.9])
    _, ids = ids_of(frames, tw.params(high_thr=0.5, low_thr=0.1))
    assert ids == [[[1]], [[1]], [[1]], [[1]]]
    s, ids = ids_of(frames, tw.params(high_thr=0.5, low_thr=0.5))
    assert ids == [[[1]], [[1]], [[0]], [[1]]]      # the 0.2 is in neither set; the track coasts one frame and is found again
    assert s[0]["next_id"] == 2


def test_pass_2_takes_only_tracks_seen_in_the_previous_frame():
    # 0.9, nothing, 0.2: the track has misses == 1 when the low-score detection comes, so pass 2 does not offer it
    frames = [[tc.rows(tc.BOX + [0.9])], [tc.rows()], [tc.rows(tc.BOX + [0.2])], [tc.rows(tc.BOX + [0.9])]]
    _, ids = ids_of(frames, tw.params(high_thr=0.5, low_thr=0.1))
    assert ids == [[[1]], [[]], [[0]], [[1]]]


def test_linear_motion_carries_a_moving_box_over_a_missed_frame():
    """x = 10, 22, (none), 46, 58, 70 with w = 20: consecutive frames overlap 8 / 32 = 0.25 > match_thr 0.2, so frame 1 matches under
    both motions and linear learns vel = 12.  Over the missed frame the box is 24 away from the last one seen: no overlap without a
    prediction (a new id), overlap 1 with it."""
    frames = tc.moving()
    s, ids = ids_of(frames, tw.params(match_thr=0.2, motion="linear"))
    assert ids == [[[1]], [[1]], [[]], [[1]], [[1]], [[1]]]
    assert s[0]["tracks"][0]["vel"].tolist() == [12.0, 0.0]
    _, ids = ids_of(frames, tw.params(match_thr=0.2, motion="none"))
    assert ids == [[[1]], [[1]], [[]], [[2]], [[2]], [[2]]]


def test_a_track_dies_in_frame_max_age_plus_1_of_absence():
    max_age = 2
    frames = tc.still([0.9]) + [[tc.rows()] for _ in range(max_age + 1)]
    p = tw.params(max_age=max_age)
    s, _ = tc.witness(frames[:1 + max_age], p, 8)
    assert s[0]["n"] == 1 and s[0]["tracks"][0]["misses"] == max_age
    s, _ = tc.witness(frames, p, 8)
    assert s[0]["n"] == 0 and s[0]["frame"] == max_age + 2


def test_min_hits_3_shows_0_0_id():
    s, ids = ids_of(tc.still([0.9, 0.9, 0.9, 0.9]), tw.params(min_hits=3))
    assert ids == [[[0]], [[0]], [[1]], [[1]]]
    # an unconfirmed track that is missed once is gone
    s, ids = ids_of(tc.still([0.9, 0.9]) + [[tc.rows()]] + tc.still([0.9, 0.9, 0.9]), tw.params(min_hits=3))
    assert ids == [[[0]], [[0]], [[]], [[0]], [[0]], [[2]]]


def test_identical_boxes_and_identical_detections_match_by_index():
    two = tc.rows(tc.BOX + [0.9], tc.BOX + [0.8])
    for match in (tw.match_walk, tw.match_rounds):
        s, ids = tc.witness([[two], [two], [two[::-1]]], tw.params(), 8, match=match)
        assert [i[0].tolist() for i in ids] == [[1, 2], [1, 2], [1, 2]]
        assert [t["score"] for t in s[0]["tracks"]] == [0.8, 0.9]      # track 1 took detection 0 of the last frame, the 0.8


def test_more_than_1024_detections_are_skipped_and_an_overflowed_segment_is_an_empty_frame():
    r = tc.crowd(1025, 0)
    s, ids = tc.witness([[r], [None], [r]], tw.params(), 1024)
    assert s[0]["skipped"] == 2 and s[0]["n"] == 1024 and ids[1][0] is None
    assert ids[0][0][-1] == 0 and ids[2][0][-1] == 0 and np.array_equal(ids[0][0], ids[2][0])
    assert all(t["misses"] == 0 and t["hits"] == 2 for t in s[0]["tracks"])


def test_witness_slots_are_stepped_in_place_and_calls_compose():
    frames = tc.drift_stream(11, T=6, K=2)
    p = tw.params(match_thr=0.1, max_age=1)
    whole, ids = tc.witness(frames, p, 16)
    slots, i1 = tc.witness(frames[:2], p, 16)
    keep = copy.deepcopy(slots)
    _, i2 = tc.witness(frames[2:], p, 16, slots=slots)
    base = np.zeros(tw.state_layout(2, 16)[3], np.uint8)
    assert np.array_equal(tw.state_bytes(whole, 16, base), tw.state_bytes(slots, 16, base))
    assert not np.array_equal(tw.state_bytes(keep, 16, base), tw.state_bytes(slots, 16, base))
    assert all(np.array_equal(x, y) for fa, fb in zip(ids, i1 + i2) for x, y in zip(fa, fb))
