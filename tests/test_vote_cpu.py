"""Box voting behind the merge (mscnn_detections_merge_vote_fwd, Net.set_box_voting) without a GPU: every refusal through the C ABI
with pointers nobody may touch and a NULL stream (each is decided before the launch and names the offending value), the sticky
Net-level setting on a graph-only net, the driver flag, the documents, and the float witness (tests/vote_witness.py) against
hand-computed cases and against its exact-rational twin.

The bound of the float witness against the exact mean is derived, not tuned.  Inputs have prob > 0 and non-negative coordinates, so
every sum runs over terms of one sign and no cancellation occurs.  With u = 2^-53 and n voters: each product p * v carries one
rounding (1 + d), |d| <= u; a sum of n same-sign terms in ANY order carries at most n - 1 roundings per term, so numerator and
denominator are within (1 + u)^n resp. (1 + u)^(n - 1) of their exact values; the division adds one more.  The quotient is therefore
within (1 + u)^(2n) - 1 of the exact one, which is below (2n + 8) u for every n the tests use (the 8 covers the second-order terms:
(1 + u)^(2n) - 1 < 2n u (1 + 2n u) and 2n u < 2^-40)."""
import ctypes as C
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

import merge_witness as mw
import nms_witness
import vote_witness as vw
from mscnn_amd import hipapi, net as mnet, zoo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
FAKE = C.c_void_p(0x1000)          # 16-byte aligned, never dereferenced: every call below is refused first
U = Fraction(1, 2 ** 53)


def L():
    return hipapi.lib()


def err():
    return L().mscnn_last_error().decode()


def vote(thr=0.5, S=4, cand=FAKE, cap=300, pack=FAKE, params="default"):
    p = C.byref(hipapi.VoteParams(thr)) if params == "default" else params
    return L().mscnn_detections_merge_vote_fwd(p, S, cand, cap, pack, None)


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_vote_params_mirror_matches_the_header_and_the_entry_points_are_exported():
    text = open(os.path.join(ROOT, "include/mscnn_hip.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\}\s*mscnn_vote_params;", text)
    assert m and [d.strip() for d in m.group(1).split(";") if d.strip()] == ["double thr"]
    assert hipapi.VoteParams._fields_ == [("thr", C.c_double)] and C.sizeof(hipapi.VoteParams) == 8
    assert hasattr(L(), "mscnn_detections_merge_vote_fwd")
    for name in ("mscnn_net_set_box_voting", "mscnn_net_get_box_voting"):
        assert hasattr(mnet.lib(), name), name
    assert re.search(r"detections_merge_vote_fwd\s+cand, pack_dev 16: refuses", text), "the op's line of the ALIGNMENT table"


def test_vote_refusals_name_the_value():
    assert vote(params=None) != 0 and "detections_merge_vote: null pointer" in err()
    assert vote(cand=None) != 0 and "null pointer" in err()
    assert vote(pack=None) != 0 and "null pointer" in err()
    assert vote(S=0) != 0 and "detections_merge_vote: 0 segments" in err()
    assert vote(S=-2) != 0 and "-2 segments" in err()
    assert vote(cap=0) != 0 and "cand_cap 0" in err()
    assert vote(cap=-7) != 0 and "cand_cap -7" in err()
    assert vote(S=1 << 16, cap=1 << 16) != 0 and f"{1 << 16} segments x {1 << 16} slots is past 2^31 - 1" in err()
    for which in ("cand", "pack"):
        assert vote(**{which: C.c_void_p(0x1008)}) != 0 and "must be 16-byte aligned" in err() and which in err(), which


@pytest.mark.parametrize("thr,text", [(NAN, "thr nan"), (0.0, "thr 0 "), (1.0, "thr 1 "), (-0.25, "thr -0.25"), (1.5, "thr 1.5"),
                                      (float("inf"), "thr inf")])
def test_vote_refuses_a_threshold_that_is_nan_or_outside_the_open_interval(thr, text):
    assert vote(thr=thr) != 0
    assert "detections_merge_vote: " + text in err() and "outside (0, 1)" in err(), err()


# ---- the Net-level setting on a graph-only net ---------------------------------------------------------------------------------------------------
def test_net_box_voting_is_off_by_default_sticky_and_unchanged_by_a_refused_value():
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=96, width=320), device=-1)
    assert n.get_box_voting() is None
    n.set_box_voting(0.5)
    assert n.get_box_voting() == 0.5
    n.set_nms(type="max")                                    # (another sticky setting does not touch this one)
    assert n.get_box_voting() == 0.5
    for bad, text in ((1.0, "thr 1 "), (-0.1, "thr -0.1"), (NAN, "thr nan"), (7.0, "thr 7 ")):
        with pytest.raises(mnet.NetError, match="set_box_voting: " + re.escape(text)):
            n.set_box_voting(bad)
        assert n.get_box_voting() == 0.5, bad
    n.set_box_voting(0.3)
    assert n.get_box_voting() == 0.3
    n.set_box_voting(None)
    assert n.get_box_voting() is None
    n.set_box_voting(0.7)
    n.set_box_voting(0)
    assert n.get_box_voting() is None
    thr = C.c_double(-1.0)
    assert mnet.lib().mscnn_net_get_box_voting(n._h, C.byref(thr)) == 0 and thr.value == 0.0
    assert mnet.lib().mscnn_net_get_box_voting(n._h, None) != 0


def test_driver_vote_flag_parses():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import run_cascademscnn
        import run_mscnn_detection
    finally:
        sys.path.pop(0)
    for mod, model in ((run_mscnn_detection, "caltech/mscnn-7s-480"), (run_cascademscnn, "kitti_car/cascade-mscnn-7s-576-2x")):
        base = ["--model", model, "--synthetic", "1"]
        assert mod.parse_args(base).vote is None
        assert mod.parse_args(base + ["--vote"]).vote == 0.5
        assert mod.parse_args(base + ["--vote", "0.3", "--flip"]).vote == 0.3
        a = mod.parse_args(base + ["--scales", "384x1280", "--vote"])
        assert a.vote == 0.5 and a.scales == [(384, 1280)]
        for bad in (["--vote", "0"], ["--vote", "1"], ["--vote", "-0.5"], ["--vote", "nan"], ["--vote", "--batch", "2"]):
            with pytest.raises(SystemExit):
                mod.parse_args(base + bad)


def test_docs_describe_the_vote_and_say_that_there_is_no_pin_on_the_reference():
    for doc in ("include/mscnn_hip.h", "include/mscnn_net.h", "DESIGN.md", "INTEGRATION.md"):
        text = " ".join(open(os.path.join(ROOT, doc)).read().split())
        m = re.search(r"[^.]*neither merge nor vote[^.]*\.", text)
        assert m, doc
        assert "no pin on the reference" in text[max(0, m.start() - 200):m.end()].lower(), doc
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--vote" in readme
    header = open(os.path.join(ROOT, "include/mscnn_hip.h")).read()
    assert "not idempotent" in header and "SUMMATION ORDER" in header


# ---- the float witness by hand ---------------------------------------------------------------------------------------------------------------
def test_voter_test_is_the_nms_overlap_with_the_threshold_included():
    A = [10.0, 10.0, 20.0, 20.0]
    cand = np.array([[10.0, 10.0, 20.0, 20.0, 0.9],          # itself: 1
                     [20.0, 10.0, 20.0, 20.0, 0.8],          # half shifted: 200 / 600 = 1 / 3
                     [30.0, 10.0, 20.0, 20.0, 0.7],          # touching: iw = 0, skipped
                     [10.0, 15.0, 20.0, 20.0, 0.6],          # 300 / 500 = 0.6
                     [12.0, 12.0, -5.0, 20.0, 0.5],          # negative width: iw < 0
                     [10.0, 10.0, 20.0, 60.0, 0.4]])         # 400 / 1200 = 1 / 3
    assert vw.voter_mask(A, cand, 0.5).tolist() == [True, False, False, True, False, False]
    assert vw.voter_mask(A, cand, 0.6).tolist() == [True, False, False, True, False, False]      # >=, not >
    third = 200.0 / 600.0
    assert vw.voter_mask(A, cand, third).tolist() == [True, True, False, True, False, True]
    assert vw.voter_mask(A, cand, np.nextafter(third, 1.0)).tolist() == [True, False, False, True, False, False]
    # the ratio is nms_witness.overlaps' (the NMS's own union form), bit for bit
    for j in (1, 3, 5):
        o = nms_witness.overlaps(np.array([A + [1.0], cand[j]]))[0, 1]
        assert vw.voter_mask(A, cand[j:j + 1], o)[0] and not vw.voter_mask(A, cand[j:j + 1], np.nextafter(o, 1.0))[0]
    # a NaN ratio does not vote (0 / 0 can not occur behind the skips; a NaN width can: fmin drops it from iw, the area keeps it)
    assert vw.voter_mask(A, [[10.0, 10.0, NAN, 20.0, 0.9]], 0.1).tolist() == [False]


def test_vote_by_hand_and_the_rows_that_stay():
    cand = np.array([[10.0, 10.0, 20.0, 20.0, 0.5],
                     [12.0, 10.0, 20.0, 20.0, 0.25],         # 360 / 440 with row 0
                     [100.0, 100.0, 20.0, 20.0, 0.75],       # alone
                     [14.0, 10.0, 20.0, 24.0, 0.25]])        # 320 / 560 = 0.571 with row 0; 0.62 with row 1
    dets = cand[[2, 0]]
    out, who = vw.vote(dets, cand, 0.5)
    assert [w.tolist() for w in who] == [[2], [0, 1, 3]]
    assert out[0].tolist() == dets[0].tolist()                                       # fewer than two voters: as it came
    # weights 0.5, 0.25, 0.25 are powers of two: every product and sum is exact
    assert out[1].tolist() == [(5 + 3 + 3.5) / 1.0, 10.0, 20.0, (10 + 5 + 6) / 1.0, 0.5]
    assert out[1, 4] == dets[1, 4]                                                   # prob untouched
    out, who = vw.vote(dets, cand, 0.9)                                              # nothing but itself anywhere
    assert np.array_equal(out, dets) and [len(w) for w in who] == [1, 1]
    zero = cand.copy()
    zero[:, 4] = 0.0                                                                 # sum p not > 0: the row stays
    assert np.array_equal(vw.vote(zero[[0]], zero, 0.5)[0], zero[[0]])
    assert vw.vote(np.zeros((0, 5)), cand, 0.5)[0].shape == (0, 5)


def test_summation_order_is_by_slot_modulo_64_then_the_butterfly():
    """Weights and values chosen so that the order shows: a big term and many small ones that vanish one at a time against it but
    not when they are added up first."""
    n = 128
    cand = np.zeros((n, 5))
    cand[:, 4] = 1.0
    cand[:, 0] = 1.0                                   # x: 1, and in slot 0 2^53
    cand[0, 0] = 2.0 ** 53
    sp, mean, voters = vw.weighted_mean(cand, range(n))
    # partial 0: 2^53 + 1 (slots 0, 64) = 2^53 in float64: that one is lost.  The other 63 partials hold 2 (slots l, l + 64); the
    # butterfly hands partial 0 the even numbers 2, 4, 8, 16, 32, 64, each of which 2^53 + ... takes in exactly: 126 arrive
    assert voters == n and sp == 128.0 and mean[0] == (2.0 ** 53 + 126.0) / 128.0
    seq = 2.0 ** 53
    for _ in range(n - 1):
        seq = seq + 1.0
    assert seq == 2.0 ** 53 and mean[0] != seq / 128.0  # one running sum in slot order would have lost every one of them
    # the voters of a partial are added in ascending slot order: 2^53 in slot 64 meets slot 0's one first, and slot 128's after it
    cand = np.zeros((129, 5))
    cand[:, 4] = 1.0
    cand[[0, 128], 0] = 1.0
    cand[64, 0] = 2.0 ** 53
    assert vw.weighted_mean(cand, [0, 64, 128])[1][0] == 2.0 ** 53 / 3.0      # (1 + 2^53) + 1: both ones lost; 2^53 + (1 + 1) would keep them


# ---- the float witness against the exact one ----------------------------------------------------------------------------------------------------
def clustered(n, rng, passes=2):
    xy = np.stack([60 + 200 * rng.integers(0, 4, n), 40 + 150 * rng.integers(0, 2, n)], 1) + rng.uniform(-6, 6, (n, 2))
    wh = rng.choice([24.0, 32.0, 48.0], (n, 2)) + rng.uniform(0, 3, (n, 2))
    prob = rng.uniform(0.01, 0.99, (n, 1)).astype(np.float32).astype(np.float64)
    rows = np.concatenate([xy, wh, prob], 1)
    cut = np.linspace(0, n, passes + 1).astype(int)
    return [(rows[a:b], np.arange(b - a, dtype=np.int32)) for a, b in zip(cut[:-1], cut[1:])]


@pytest.mark.parametrize("n,thr,seed", [(40, 0.5, 1), (200, 0.3, 2), (700, 0.5, 3), (700, 0.1, 4)])
def test_float_witness_is_within_the_derived_bound_of_the_exact_mean(n, thr, seed):
    passes = clustered(n, np.random.default_rng(seed))
    dets, voted, pas, row, cands, who, cand_pass = vw.vote_segment(passes, thr)
    cand, _ = vw.candidates_of(passes)
    assert cands == n and np.all(cand[:, 4] > 0) and np.all(cand[:, :4] >= 0)
    multi, higher, lonely = vw.vote_facts(dets, cand, cand_pass, who)
    assert multi and higher, "the case shows nothing"
    most = max(len(w) for w in who)
    assert most >= 4 and (most > 64 or thr != 0.1), most      # (the last case: more than one voter in a partial sum)
    checked = 0
    for k, slots in enumerate(who):
        assert dets[k, 4] == voted[k, 4]
        if len(slots) < 2:
            assert np.array_equal(dets[k].view(np.uint64), voted[k].view(np.uint64))
            continue
        exact = vw.vote_exact(cand, slots)
        bound = (2 * len(slots) + 8) * U
        for q in range(4):
            got = Fraction(float(voted[k, q]))
            assert abs(got - exact[q]) <= bound * exact[q], (k, q, len(slots), float(abs(got - exact[q]) / exact[q]) * 2.0 ** 53)
        checked += 1
    assert checked >= 5


def test_vote_segment_keeps_the_merge_witness_result_beside_the_voted_one():
    passes = clustered(60, np.random.default_rng(9), passes=3)
    dets, voted, pas, row, cands, who, cand_pass = vw.vote_segment(passes, 0.5)
    wd, wp, wr, wc = mw.merge(passes)
    assert np.array_equal(dets, wd) and np.array_equal(pas, wp) and np.array_equal(row, wr) and cands == wc == 60
    assert cand_pass.tolist() == [0] * 20 + [1] * 20 + [2] * 20
    assert not np.array_equal(dets, voted) and np.array_equal(dets[:, 4], voted[:, 4])
    # every kept row votes for itself (overlap 1 with its own slot)
    cand, _ = vw.candidates_of(passes)
    for k, slots in enumerate(who):
        assert any(np.array_equal(cand[j], dets[k]) for j in slots)
