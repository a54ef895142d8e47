"""Soft-NMS over the merged candidates (mscnn_detections_merge_soft_fwd, Net.set_soft_nms) without a GPU: every refusal through the C
ABI with pointers nobody may touch and a NULL stream (each is decided before any launch and names the offending value), the workspace
sizes, the sticky Net-level setting on a graph-only net, the driver flags, the documents, and the float witness
(tests/soft_witness.py) against hand-computed cases and against its exact-rational twin.

The bound of the float witness's scores against the exact ones is derived in soft_witness.soft_exact, not tuned: on boxes with small
integer coordinates the overlap r = o / u is ONE rounding, so a decay s (1 - r) costs at most (r / (1 - r) + 2) 2^-53 relative, and a
pick's score went through at most D of them."""
import ctypes as C
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

import soft_witness as sw
from mscnn_amd import hipapi, net as mnet, zoo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
FAKE = C.c_void_p(0x1000)          # 16-byte aligned, never dereferenced: every call below is refused first


def L():
    return hipapi.lib()


def err():
    return L().mscnn_last_error().decode()


def soft(method=1, sigma=0.5, score_thr=0.001, max_out=0, S=4, cand=FAKE, cap=300, pack=FAKE, ws=FAKE, ws_bytes=None, overlap="default",
         params="default"):
    p = C.byref(hipapi.SoftNmsParams(method, sigma, score_thr, max_out)) if params == "default" else params
    ov = (C.c_double * max(S, 1))(*([0.5] * max(S, 1))) if overlap == "default" else overlap
    wb = L().mscnn_detections_merge_soft_workspace_bytes(S, cap) if ws_bytes is None else ws_bytes
    return L().mscnn_detections_merge_soft_fwd(ov, p, S, cand, cap, pack, ws, C.c_size_t(wb), None)


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_soft_params_mirror_matches_the_header_and_the_entry_points_are_exported():
    text = open(os.path.join(ROOT, "include/mscnn_hip.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\}\s*mscnn_soft_nms_params;", text)
    assert m and [d.strip() for d in m.group(1).split(";") if d.strip()] == ["int method", "double sigma", "double score_thr", "int max_out"]
    assert hipapi.SoftNmsParams._fields_ == [("method", C.c_int), ("sigma", C.c_double), ("score_thr", C.c_double), ("max_out", C.c_int)]
    assert C.sizeof(hipapi.SoftNmsParams) == 32
    assert re.search(r"MSCNN_SOFT_NMS_LINEAR = 1, MSCNN_SOFT_NMS_GAUSSIAN = 2", text) and hipapi.SOFT_NMS_METHODS == dict(linear=1, gaussian=2)
    for name in ("mscnn_detections_merge_soft_fwd", "mscnn_detections_merge_soft_workspace_bytes"):
        assert hasattr(L(), name), name
    for name in ("mscnn_net_set_soft_nms", "mscnn_net_get_soft_nms"):
        assert hasattr(mnet.lib(), name), name
    assert re.search(r"detections_merge_soft_fwd\s+cand, workspace, pack_dev 16: refuses", text), "the op's line of the ALIGNMENT table"


def test_soft_refusals_name_the_value():
    assert soft(params=None) != 0 and "detections_merge_soft: null pointer" in err()
    for which in ("cand", "pack", "ws", "overlap"):
        assert soft(**{which: None}) != 0 and "detections_merge_soft: null pointer" in err(), which
    assert soft(S=0, ws_bytes=1 << 20) != 0 and "detections_merge_soft: 0 segments" in err()
    assert soft(S=-2, ws_bytes=1 << 20) != 0 and "-2 segments" in err()
    assert soft(cap=0, ws_bytes=1 << 20) != 0 and "cand_cap 0" in err()
    assert soft(cap=-7, ws_bytes=1 << 20) != 0 and "cand_cap -7" in err()
    assert soft(S=1 << 16, cap=1 << 16, ws_bytes=1 << 20) != 0 and f"{1 << 16} segments x {1 << 16} slots is past 2^31 - 1" in err()
    for method in (0, 3, -1):
        assert soft(method=method) != 0 and f"detections_merge_soft: method {method} is neither 1 (linear) nor 2 (gaussian)" in err()
    for max_out in (-1, -300):
        assert soft(max_out=max_out) != 0 and f"detections_merge_soft: max_out {max_out}" in err()
    for which, name in (("cand", "cand"), ("ws", "workspace"), ("pack", "pack_dev")):
        assert soft(**{which: C.c_void_p(0x1008)}) != 0 and f"detections_merge_soft: {name} must be 16-byte aligned" in err(), which


@pytest.mark.parametrize("sigma,text", [(NAN, "sigma nan"), (0.0, "sigma 0 "), (-0.5, "sigma -0.5"), (INF, "sigma inf")])
def test_gaussian_refuses_a_sigma_that_is_not_finite_or_not_positive(sigma, text):
    assert soft(method=2, sigma=sigma) != 0
    assert "detections_merge_soft: " + text in err() and "not a finite value > 0" in err(), err()
    assert soft(method=1, sigma=sigma, cand=C.c_void_p(0x1008)) != 0 and "cand must be 16-byte aligned" in err(), "linear does not read sigma"


@pytest.mark.parametrize("thr,text", [(NAN, "score_thr nan"), (-0.001, "score_thr -0.001"), (INF, "score_thr inf"), (-INF, "score_thr -inf")])
def test_soft_refuses_a_score_threshold_that_is_nan_infinite_or_negative(thr, text):
    for method in (1, 2):
        assert soft(method=method, score_thr=thr) != 0
        assert "detections_merge_soft: " + text in err() and "not a finite value >= 0" in err(), err()


def test_a_nan_overlap_is_refused_with_linear_and_not_read_with_gaussian():
    ov = (C.c_double * 4)(0.5, 0.5, NAN, 0.5)
    assert soft(method=1, overlap=ov) != 0 and "detections_merge_soft: segment 2: nms_overlap is NaN" in err()
    # gaussian does not read the overlaps: the call gets as far as the next refusal
    assert soft(method=2, overlap=ov, cand=C.c_void_p(0x1008)) != 0 and "cand must be 16-byte aligned" in err()


def test_workspace_bytes_and_the_refusal_of_a_short_workspace():
    wsb = L().mscnn_detections_merge_soft_workspace_bytes
    for S, cap in ((0, 10), (-1, 10), (4, 0), (4, -3), (1 << 16, 1 << 16)):
        assert wsb(S, cap) == 0, (S, cap)
    for S, cap in ((1, 1), (33, 4032), (1, 8000)):
        assert wsb(S, cap) > 0, (S, cap)
    # a list of up to 4096 slots lives in registers; a longer one needs 8 + 1 bytes per slot for each list of a launch (32 at the most)
    assert wsb(1, 4096) == wsb(33, 4032) == wsb(1, 1) and wsb(1, 4097) >= 9 * 4097 and wsb(1, 8000) >= 9 * 8000
    assert wsb(2, 8000) == 2 * wsb(1, 8000) and wsb(33, 8000) == wsb(32, 8000) == 32 * wsb(1, 8000)
    need = wsb(4, 8000)
    assert soft(cap=8000, ws_bytes=need - 1) == 3, "MSCNN_ERR_WORKSPACE"
    assert f"detections_merge_soft: workspace {need - 1} < {need}" in err()
    assert soft(cap=300, ws_bytes=0) == 3 and "workspace 0 <" in err()


# ---- the Net-level setting on a graph-only net ---------------------------------------------------------------------------------------------------
def test_net_soft_nms_is_off_by_default_sticky_and_unchanged_by_a_refused_value():
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=96, width=320), device=-1)
    assert n.get_soft_nms() is None
    n.set_soft_nms("gaussian", sigma=0.3, score_thr=0.01, max_out=100)
    want = dict(method="gaussian", sigma=0.3, score_thr=0.01, max_out=100)
    assert n.get_soft_nms() == want
    n.set_nms(type="max")                                    # (other sticky settings do not touch this one)
    n.set_box_voting(0.5)
    assert n.get_soft_nms() == want and n.get_box_voting() == 0.5
    bad = [(dict(method=3), "method 3 "), (dict(method=-1), "method -1 "), (dict(method="gaussian", sigma=0.0), "sigma 0 "),
           (dict(method="gaussian", sigma=NAN), "sigma nan"), (dict(method="gaussian", sigma=INF), "sigma inf"),
           (dict(method="linear", score_thr=-0.5), "score_thr -0.5"), (dict(method="linear", score_thr=NAN), "score_thr nan"),
           (dict(method="linear", score_thr=INF), "score_thr inf"), (dict(method="linear", max_out=-1), "max_out -1"),
           (dict(method=None, max_out=-1), "max_out -1")]
    for kw, text in bad:
        with pytest.raises(mnet.NetError, match="set_soft_nms: " + re.escape(text)):
            n.set_soft_nms(**kw)
        assert n.get_soft_nms() == want, kw
    with pytest.raises(mnet.NetError, match="set_soft_nms: method 'cubic'"):
        n.set_soft_nms("cubic")
    assert n.get_soft_nms() == want
    n.set_soft_nms("linear")
    assert n.get_soft_nms() == dict(method="linear", sigma=0.5, score_thr=0.001, max_out=0)
    n.set_soft_nms(None)
    assert n.get_soft_nms() is None and n.get_box_voting() == 0.5
    m, mo, sg, th = C.c_int(-1), C.c_int(-1), C.c_double(-1.0), C.c_double(-1.0)
    assert mnet.lib().mscnn_net_get_soft_nms(n._h, C.byref(m), C.byref(sg), C.byref(th), C.byref(mo)) == 0 and m.value == 0
    assert mnet.lib().mscnn_net_get_soft_nms(n._h, None, C.byref(sg), C.byref(th), C.byref(mo)) != 0


def test_driver_soft_nms_flags_parse(capsys):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import run_cascademscnn
        import run_mscnn_detection
    finally:
        sys.path.pop(0)
    for mod, model in ((run_mscnn_detection, "caltech/mscnn-7s-480"), (run_cascademscnn, "kitti_car/cascade-mscnn-7s-576-2x")):
        base = ["--model", model, "--synthetic", "1"]
        a = mod.parse_args(base)
        assert a.soft_nms is None and a.soft_thr == 0.001 and a.max_dets == 0
        assert mod.parse_args(base + ["--soft-nms", "linear"]).soft_nms == ("linear", 0.5)
        assert mod.parse_args(base + ["--soft-nms", "gaussian"]).soft_nms == ("gaussian", 0.5)
        a = mod.parse_args(base + ["--soft-nms", "gaussian:0.3", "--soft-thr", "0.01", "--max-dets", "300", "--flip", "--vote"])
        assert a.soft_nms == ("gaussian", 0.3) and a.soft_thr == 0.01 and a.max_dets == 300 and a.vote == 0.5
        for bad in (["--soft-nms", "cubic"], ["--soft-nms", "linear:0.5"], ["--soft-nms", "gaussian:0"], ["--soft-nms", "gaussian:nan"],
                    ["--soft-nms", "gaussian:x"], ["--soft-thr", "0.1"], ["--max-dets", "10"], ["--soft-nms", "linear", "--soft-thr", "-1"],
                    ["--soft-nms", "linear", "--max-dets", "-1"], ["--soft-nms", "linear", "--batch", "2"]):
            with pytest.raises(SystemExit):
                mod.parse_args(base + bad)
    capsys.readouterr()


def test_docs_describe_soft_nms_and_say_that_there_is_no_pin_on_the_reference():
    for doc in ("include/mscnn_hip.h", "include/mscnn_net.h", "DESIGN.md", "INTEGRATION.md"):
        text = " ".join(open(os.path.join(ROOT, doc)).read().split())
        m = re.search(r"[^.]*neither merge nor decay a score[^.]*\.", text)
        assert m, doc
        assert "no pin on the reference" in text[max(0, m.start() - 200):m.end()].lower(), doc
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--soft-nms" in readme and "profiles/detect_merge_soft.txt" in readme
    header = open(os.path.join(ROOT, "include/mscnn_hip.h")).read()
    assert "TOTAL order" in header and "lowest slot" in header


# ---- the float witness by hand ---------------------------------------------------------------------------------------------------------------
HAND = np.array([[10.0, 10.0, 20.0, 20.0, 0.5],          # slot 0
                 [20.0, 10.0, 20.0, 20.0, 0.75],         # slot 1: 200 / 600 = 1 / 3 with slot 0
                 [10.0, 15.0, 20.0, 20.0, 0.625],        # slot 2: 300 / 500 = 0.6 with slot 0, 150 / 650 with slot 1
                 [100.0, 100.0, 20.0, 20.0, 0.25],       # slot 3: alone
                 [30.0, 10.0, 20.0, 20.0, 0.5]])         # slot 4: touches slot 0 (iw = 0), 1 / 3 with slot 1; prob equal to slot 0's


def test_linear_by_hand_decay_order_threshold_and_the_tie_rule():
    # overlap 0.5: pick 1 (0.75) decays nobody (1/3, 150/650, 1/3 are all under 0.5); pick 2 (0.625) decays slot 0 by 1 - 0.6:
    # 0.5 * 0.4; then slots 0 (0.2) and 4 (0.5) and 3 (0.25): 4, 3, 0
    d, slots, decays, gap = sw.soft(HAND, sw.LINEAR, overlap=0.5, score_thr=0.001)
    assert slots.tolist() == [1, 2, 4, 3, 0] and decays == 1
    assert d[:, 4].tolist() == [0.75, 0.625, 0.5, 0.25, 0.5 * (1.0 - 300.0 / 500.0)]
    assert np.array_equal(d[:, :4], HAND[slots, :4])
    # overlap 0.3: pick 1 decays slots 0 and 4 by 1 - 1/3 (both to the same bits); pick 2 decays slot 0 once more; then 4, 3, 0
    d, slots, decays, gap = sw.soft(HAND, sw.LINEAR, overlap=0.3, score_thr=0.001)
    s0 = 0.5 * (1.0 - 200.0 / 600.0)
    assert slots.tolist() == [1, 2, 4, 3, 0] and decays == 3
    assert d[:, 4].tolist() == [0.75, 0.625, s0, 0.25, s0 * (1.0 - 300.0 / 500.0)]
    # score_thr drops what is under it, max_out cuts the sequence
    assert sw.soft(HAND, sw.LINEAR, overlap=0.5, score_thr=0.3)[1].tolist() == [1, 2, 4]
    assert sw.soft(HAND, sw.LINEAR, overlap=0.5, score_thr=0.001, max_out=2)[1].tolist() == [1, 2]
    assert sw.soft(HAND, sw.LINEAR, overlap=0.5, score_thr=0.8)[1].tolist() == []
    assert sw.soft(np.zeros((0, 5)), sw.LINEAR)[0].shape == (0, 5)
    # equal scores from the start: the lower slot first
    tie = HAND[[0, 4, 3]].copy()
    tie[:, 4] = 0.5
    assert sw.soft(tie, sw.LINEAR, overlap=0.5)[1].tolist() == [0, 1, 2]
    # a NaN score ranks below every number and ends the picking when it is the best that is left
    nan = HAND.copy()
    nan[1, 4] = NAN
    assert sw.soft(nan, sw.LINEAR, overlap=0.5, score_thr=0.0)[1].tolist() == [2, 4, 3, 0]


def test_gaussian_by_hand_decays_every_overlapping_candidate():
    d, slots, decays, gap = sw.soft(HAND, sw.GAUSSIAN, sigma=0.5, score_thr=0.001)
    third, r12 = 200.0 / 600.0, 150.0 / 650.0
    s0 = 0.5 * np.exp(-(third * third) / 0.5)
    s2 = 0.625 * np.exp(-(r12 * r12) / 0.5)
    assert slots[0] == 1 and decays >= 3
    # after pick 1: slot 2 = s2 (0.562), slots 0 and 4 = s0 (0.400, a tie), slot 3 = 0.25: pick 2, which decays slot 0 once more
    # (numpy's exp on an array and on a scalar may differ in the last place: two ulps of room)
    near = lambda a, b: abs(a - b) <= 2 * np.spacing(b)      # noqa: E731
    assert slots.tolist() == [1, 2, 4, 3, 0] and near(d[1, 4], s2) and near(d[2, 4], s0) and d[3, 4] == 0.25
    assert near(d[4, 4], s0 * np.exp(-(0.6 * 0.6) / 0.5))
    # the overlap threshold is not read
    assert np.array_equal(sw.soft(HAND, sw.GAUSSIAN, overlap=0.9, sigma=0.5)[0], sw.soft(HAND, sw.GAUSSIAN, overlap=0.1, sigma=0.5)[0])


# ---- the float witness against the exact one ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,overlap,thr,max_out,seed", [(60, 0.3, 0.05, 0, 1), (60, 0.5, 0.001, 0, 2), (200, 0.3, 0.02, 40, 3)])
def test_float_witness_is_within_the_derived_bound_of_the_exact_scores(n, overlap, thr, max_out, seed):
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 8, n)
    cand = np.stack([100 + 60 * (m % 4) + rng.integers(-5, 6, n), 100 + 60 * (m // 4) + rng.integers(-5, 6, n), rng.choice([28, 32, 36], n),
                     rng.choice([28, 32, 36], n), rng.uniform(0.05, 1, n).astype(np.float32)], 1).astype(np.float64)
    assert np.all(cand[:, :4] == np.round(cand[:, :4])) and np.all(np.abs(cand[:, :4]) < 2 ** 20), "the bound's premise: integer boxes"
    d, slots, decays, gap = sw.soft(cand, sw.LINEAR, overlap=overlap, score_thr=thr, max_out=max_out)
    decayed, dropped, reordered = sw.soft_facts(cand, d, slots, decays)
    assert decayed and dropped and reordered, "the case shows nothing"
    assert gap > 1e-9, "a pick of this input hangs on the last bits"
    eslots, escores, bounds = sw.soft_exact(cand, overlap=overlap, score_thr=thr, max_out=max_out)
    D = len(slots)
    assert D >= 20 and (max_out == 0 or D == max_out) and slots.tolist() == eslots, "the same picks in the same order"
    worst = 0.0
    for k in range(D):
        got = Fraction(float(d[k, 4]))
        assert abs(got - escores[k]) <= Fraction(bounds[k]) * escores[k], (k, float(abs(got - escores[k]) / escores[k]) * 2.0 ** 53, bounds[k] * 2.0 ** 53)
        worst = max(worst, bounds[k])
    assert 0 < worst < 64 * D * 2.0 ** -53, "a pick's score went through at most D decays of a few roundings each"
