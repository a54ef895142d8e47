"""Matrix NMS over the merged candidates (mscnn_detections_merge_matrix_fwd, Net.set_matrix_nms) without a GPU: the ABI as a C
compiler sees it, every refusal through the library with pointers nobody may touch and a NULL stream (each is decided before any
launch and names the offending value), the workspace sizes, the sticky Net-level setting on a graph-only net and its mutual exclusion
with Soft-NMS, the driver flags, the documents, and the witnesses of tests/matrix_witness.py against each other.

The bound of the float witness's scores against the exact ones is derived in matrix_witness.matrix_exact, not tuned."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import matrix_witness as xw
from mscnn_amd import hipapi, net as mnet, zoo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
FAKE = C.c_void_p(0x1000)          # 16-byte aligned, never dereferenced: every call below is refused first


def L():
    return hipapi.lib()


def err():
    return L().mscnn_last_error().decode()


def matrix(method=1, sigma=0.5, score_thr=0.001, max_out=0, S=4, cand=FAKE, cap=300, pack=FAKE, ws=FAKE, ws_bytes=None, params="default"):
    p = C.byref(hipapi.MatrixNmsParams(method, sigma, score_thr, max_out)) if params == "default" else params
    wb = L().mscnn_detections_merge_matrix_workspace_bytes(S, cap) if ws_bytes is None else ws_bytes
    return L().mscnn_detections_merge_matrix_fwd(p, S, cand, cap, pack, ws, C.c_size_t(wb), None)


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_matrix_params_mirror_matches_the_header_and_the_entry_points_are_exported():
    text = open(os.path.join(ROOT, "include/mscnn_hip.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\}\s*mscnn_matrix_nms_params;", text)
    assert m and [d.strip() for d in m.group(1).split(";") if d.strip()] == ["int method", "double sigma", "double score_thr", "int max_out"]
    assert hipapi.MatrixNmsParams._fields_ == [("method", C.c_int), ("sigma", C.c_double), ("score_thr", C.c_double), ("max_out", C.c_int)]
    assert C.sizeof(hipapi.MatrixNmsParams) == 32
    assert [getattr(hipapi.MatrixNmsParams, f).offset for f in ("method", "sigma", "score_thr", "max_out")] == [0, 8, 16, 24]
    assert re.search(r"MSCNN_MATRIX_NMS_LINEAR = 1, MSCNN_MATRIX_NMS_GAUSSIAN = 2", text) and hipapi.MATRIX_NMS_METHODS == dict(linear=1, gaussian=2)
    for name in ("mscnn_detections_merge_matrix_fwd", "mscnn_detections_merge_matrix_workspace_bytes"):
        assert hasattr(L(), name), name
    for name in ("mscnn_net_set_matrix_nms", "mscnn_net_get_matrix_nms"):
        assert hasattr(mnet.lib(), name), name
    assert re.search(r"detections_merge_matrix_fwd\s+cand, workspace, pack_dev 16: refuses", text), "the op's line of the ALIGNMENT table"
    vp, ci = C.c_void_p, C.c_int
    assert L().mscnn_detections_merge_matrix_fwd.argtypes == [vp, ci, vp, ci, vp, vp, C.c_size_t, vp]
    assert L().mscnn_detections_merge_matrix_workspace_bytes.argtypes == [ci, ci]
    assert L().mscnn_detections_merge_matrix_workspace_bytes.restype == C.c_size_t
    proto = " ".join(text.split())
    assert ("int mscnn_detections_merge_matrix_fwd(const mscnn_matrix_nms_params* mx, int num_segments, void* cand, int cand_cap, "
            "void* pack_dev, void* workspace, size_t workspace_bytes, void* stream);") in proto
    assert "size_t mscnn_detections_merge_matrix_workspace_bytes(int num_segments, int cand_cap);" in proto


def test_matrix_struct_layout_as_a_c_compiler_sees_it(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or "/opt/rocm/bin/hipcc"      # (the project does not build without hipcc)
    assert shutil.which(cc) or os.path.exists(cc), "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "mscnn_hip.h"\n#include "mscnn_net.h"\n'
                   "_Static_assert(sizeof(mscnn_matrix_nms_params) == 32, \"size\");\n"
                   "_Static_assert(offsetof(mscnn_matrix_nms_params, method) == 0 && offsetof(mscnn_matrix_nms_params, sigma) == 8 && "
                   "offsetof(mscnn_matrix_nms_params, score_thr) == 16 && offsetof(mscnn_matrix_nms_params, max_out) == 24, \"offsets\");\n"
                   "_Static_assert(MSCNN_MATRIX_NMS_LINEAR == 1 && MSCNN_MATRIX_NMS_GAUSSIAN == 2, \"methods\");\n"
                   "_Static_assert(sizeof(mscnn_soft_nms_params) == 32, \"the soft params keep their size\");\n")
    r = subprocess.run([cc, "-x", "c", "-std=c11", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_matrix_refusals_name_the_value():
    assert matrix(params=None) != 0 and "detections_merge_matrix: null pointer" in err()
    for which in ("cand", "pack", "ws"):
        assert matrix(**{which: None}) != 0 and "detections_merge_matrix: null pointer" in err(), which
    assert matrix(S=0, ws_bytes=1 << 20) != 0 and "detections_merge_matrix: 0 segments" in err()
    assert matrix(S=-2, ws_bytes=1 << 20) != 0 and "-2 segments" in err()
    assert matrix(cap=0, ws_bytes=1 << 20) != 0 and "detections_merge_matrix: cand_cap 0" in err()
    assert matrix(cap=-7, ws_bytes=1 << 20) != 0 and "cand_cap -7" in err()
    assert matrix(S=1 << 16, cap=1 << 16, ws_bytes=1 << 20) != 0 and f"{1 << 16} segments x {1 << 16} slots is past 2^31 - 1" in err()
    assert matrix(S=1, cap=(1 << 30) + 1, ws_bytes=1 << 20) != 0 and f"cand_cap {(1 << 30) + 1} is past the sort's 2^30 keys" in err()
    for method in (0, 3, -1):
        assert matrix(method=method) != 0 and f"detections_merge_matrix: method {method} is neither 1 (linear) nor 2 (gaussian)" in err()
    for max_out in (-1, -300):
        assert matrix(max_out=max_out) != 0 and f"detections_merge_matrix: max_out {max_out}" in err()
    for which, name in (("cand", "cand"), ("ws", "workspace"), ("pack", "pack_dev")):
        assert matrix(**{which: C.c_void_p(0x1008)}) != 0 and f"detections_merge_matrix: {name} must be 16-byte aligned" in err(), which


@pytest.mark.parametrize("sigma,text", [(NAN, "sigma nan"), (0.0, "sigma 0 "), (-0.5, "sigma -0.5"), (INF, "sigma inf")])
def test_gaussian_refuses_a_sigma_that_is_not_finite_or_not_positive(sigma, text):
    assert matrix(method=2, sigma=sigma) != 0
    assert "detections_merge_matrix: " + text in err() and "not a finite value > 0" in err(), err()
    assert matrix(method=1, sigma=sigma, cand=C.c_void_p(0x1008)) != 0 and "cand must be 16-byte aligned" in err(), "linear does not read sigma"


@pytest.mark.parametrize("thr,text", [(NAN, "score_thr nan"), (-0.001, "score_thr -0.001"), (INF, "score_thr inf"), (-INF, "score_thr -inf")])
def test_matrix_refuses_a_score_threshold_that_is_nan_infinite_or_negative(thr, text):
    for method in (1, 2):
        assert matrix(method=method, score_thr=thr) != 0
        assert "detections_merge_matrix: " + text in err() and "not a finite value >= 0" in err(), err()


def test_workspace_bytes_are_linear_and_a_short_workspace_is_refused():
    wsb = L().mscnn_detections_merge_matrix_workspace_bytes
    for S, cap in ((0, 10), (-1, 10), (4, 0), (4, -3), (1 << 16, 1 << 16), (1, (1 << 30) + 1)):
        assert wsb(S, cap) == 0, (S, cap)
    for S, cap in ((1, 1), (33, 4032), (1, 4033), (1, 8000), (3, 20000)):
        assert wsb(S, cap) > 0, (S, cap)
    caps = [1, 2, 100, 255, 256, 257, 1000, 4032, 4033, 5000, 8192, 8193, 20000, 40000, 1 << 20]
    sizes = [wsb(1, c) for c in caps]
    assert sizes == sorted(sizes) and len(set(sizes)) > 10, "monotone in cand_cap"
    # linear, not quadratic.  This layout, per slot of a list: the sorted slice (32 + 8 + 4 bytes), the keys of the sort's power of
    # two above 4032 slots (at most 2 x 8), score' (8) and two areas of at most 8 partial rows (2 x 8 x 8) -- under 200 bytes a
    # slot where the issue's single-row layout would have 64; an n x n matrix of doubles would be 8 x 20000 = 160000 bytes a slot
    assert wsb(1, 20000) < 200 * 20000 + wsb(1, 1)
    assert wsb(1, 40000) < 2 * wsb(1, 20000) + 4096 and wsb(1, 1 << 20) < 200 * (1 << 20) + wsb(1, 1)
    assert wsb(33, 300) > wsb(32, 300) > wsb(1, 300) and wsb(5, 8000) == wsb(1, 8000), "a list above 4032 slots is served alone"
    need = wsb(4, 8000)
    assert matrix(cap=8000, ws_bytes=need - 1) == 3, "MSCNN_ERR_WORKSPACE"
    assert f"detections_merge_matrix: workspace {need - 1} < {need}" in err()
    assert matrix(cap=300, ws_bytes=0) == 3 and "workspace 0 <" in err()


# ---- the Net-level setting on a graph-only net ---------------------------------------------------------------------------------------------------
def graph_net():
    return mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=96, width=320), device=-1)


def test_net_matrix_nms_is_off_by_default_sticky_and_unchanged_by_a_refused_value():
    n = graph_net()
    assert n.get_matrix_nms() is None
    n.set_matrix_nms("gaussian", sigma=0.3, score_thr=0.01, max_out=100)
    want = dict(method="gaussian", sigma=0.3, score_thr=0.01, max_out=100)
    assert n.get_matrix_nms() == want
    n.set_nms(type="max")                                    # (other sticky settings do not touch this one)
    n.set_box_voting(0.5)
    assert n.get_matrix_nms() == want and n.get_box_voting() == 0.5 and n.get_soft_nms() is None
    bad = [(dict(method=3), "method 3 "), (dict(method=-1), "method -1 "), (dict(method="gaussian", sigma=0.0), "sigma 0 "),
           (dict(method="gaussian", sigma=NAN), "sigma nan"), (dict(method="gaussian", sigma=INF), "sigma inf"),
           (dict(method="linear", score_thr=-0.5), "score_thr -0.5"), (dict(method="linear", score_thr=NAN), "score_thr nan"),
           (dict(method="linear", score_thr=INF), "score_thr inf"), (dict(method="linear", max_out=-1), "max_out -1"),
           (dict(method=None, max_out=-1), "max_out -1")]
    for kw, text in bad:
        with pytest.raises(mnet.NetError, match="set_matrix_nms: " + re.escape(text)):
            n.set_matrix_nms(**kw)
        assert n.get_matrix_nms() == want, kw
    with pytest.raises(mnet.NetError, match="set_matrix_nms: method 'cubic'"):
        n.set_matrix_nms("cubic")
    assert n.get_matrix_nms() == want
    n.set_matrix_nms("linear")
    assert n.get_matrix_nms() == dict(method="linear", sigma=0.5, score_thr=0.001, max_out=0)
    n.set_matrix_nms(None)
    assert n.get_matrix_nms() is None and n.get_box_voting() == 0.5
    m, mo, sg, th = C.c_int(-1), C.c_int(-1), C.c_double(-1.0), C.c_double(-1.0)
    assert mnet.lib().mscnn_net_get_matrix_nms(n._h, C.byref(m), C.byref(sg), C.byref(th), C.byref(mo)) == 0 and m.value == 0
    assert mnet.lib().mscnn_net_get_matrix_nms(n._h, None, C.byref(sg), C.byref(th), C.byref(mo)) != 0


def test_matrix_nms_and_soft_nms_exclude_each_other_in_both_orders():
    n = graph_net()
    n.set_matrix_nms("linear", score_thr=0.02)
    with pytest.raises(mnet.NetError, match=r"set_soft_nms: method 2 while Matrix NMS is on \(set_matrix_nms method 1\)"):
        n.set_soft_nms("gaussian")
    assert n.get_soft_nms() is None and n.get_matrix_nms() == dict(method="linear", sigma=0.5, score_thr=0.02, max_out=0)
    n.set_soft_nms(None)                                     # (turning the other one OFF is no conflict)
    n.set_matrix_nms(None)
    n.set_soft_nms("linear", max_out=9)
    with pytest.raises(mnet.NetError, match=r"set_matrix_nms: method 2 while Soft-NMS is on \(set_soft_nms method 1\)"):
        n.set_matrix_nms("gaussian", sigma=0.25)
    assert n.get_matrix_nms() is None and n.get_soft_nms() == dict(method="linear", sigma=0.5, score_thr=0.001, max_out=9)
    n.set_matrix_nms(None)
    n.set_soft_nms(None)
    n.set_matrix_nms("gaussian", sigma=0.25)
    assert n.get_matrix_nms()["sigma"] == 0.25


def test_driver_matrix_nms_flags_parse(capsys):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import run_cascademscnn
        import run_mscnn_detection
    finally:
        sys.path.pop(0)
    for mod, model in ((run_mscnn_detection, "caltech/mscnn-7s-480"), (run_cascademscnn, "kitti_car/cascade-mscnn-7s-576-2x")):
        base = ["--model", model, "--synthetic", "1"]
        a = mod.parse_args(base)
        assert a.matrix_nms is None and a.soft_nms is None and a.soft_thr == 0.001 and a.max_dets == 0
        assert mod.parse_args(base + ["--matrix-nms", "linear"]).matrix_nms == ("linear", 0.5)
        assert mod.parse_args(base + ["--matrix-nms", "gaussian"]).matrix_nms == ("gaussian", 0.5)
        a = mod.parse_args(base + ["--matrix-nms", "gaussian:0.3", "--soft-thr", "0.01", "--max-dets", "300", "--flip", "--vote"])
        assert a.matrix_nms == ("gaussian", 0.3) and a.soft_thr == 0.01 and a.max_dets == 300 and a.vote == 0.5 and a.soft_nms is None
        for bad in (["--matrix-nms", "cubic"], ["--matrix-nms", "linear:0.5"], ["--matrix-nms", "gaussian:0"], ["--matrix-nms", "gaussian:nan"],
                    ["--matrix-nms", "linear", "--soft-nms", "linear"], ["--matrix-nms", "gaussian", "--soft-nms", "gaussian:0.3"],
                    ["--matrix-nms", "linear", "--soft-thr", "-1"], ["--matrix-nms", "linear", "--max-dets", "-1"],
                    ["--matrix-nms", "linear", "--batch", "2"]):
            with pytest.raises(SystemExit):
                mod.parse_args(base + bad)
    capsys.readouterr()


def test_docs_describe_matrix_nms_and_say_what_it_is_not():
    for doc in ("include/mscnn_hip.h", "include/mscnn_net.h", "DESIGN.md", "INTEGRATION.md"):
        text = " ".join(open(os.path.join(ROOT, doc)).read().split())
        assert "Matrix NMS" in text and "matrix_nms" in text, doc
        at = [m.start() for m in re.finditer(r"Matrix NMS", text)]
        near = lambda pat: any(re.search(pat, text[max(0, a - 1500):a + 2500], re.I) for a in at)      # noqa: E731
        assert near(r"no pin on the reference"), doc
        assert near(r"not Soft-NMS's scores|NOT return Soft-NMS's scores|not a product over picks"), doc
        assert near(r"not evaluated"), doc
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--matrix-nms" in readme and "profiles/detect_merge_matrix.txt" in readme


# ---- the witnesses against each other ---------------------------------------------------------------------------------------------------------
def clustered_list(n, rng):
    """n integer boxes in clusters of about five on a 16-column grid, float32 probs."""
    m = rng.integers(0, max(1, n // 5), n)
    xy = np.stack([120 * (m % 16) + 20, 120 * (m // 16) + 20], 1) + rng.integers(-6, 7, (n, 2))
    return np.concatenate([xy, rng.choice([14, 20, 32, 48], (n, 2)), rng.uniform(0.05, 1, (n, 1)).astype(np.float32)], 1).astype(np.float64)


DUPLICATES = np.array([[10.0, 10.0, 20.0, 20.0, 0.75],       # rank 0
                       [10.0, 10.0, 20.0, 20.0, 0.5],        # rank 1: an exact duplicate of rank 0 -> c = 1, its own terms are skipped
                       [10.0, 15.0, 20.0, 20.0, 0.25],       # rank 3: 300 / 500 = 0.6 with both
                       [10.0, 10.0, 20.0, 20.0, 0.5]])       # rank 2: the duplicate again, the later slot of equal probs


def lists_200():
    rng = np.random.default_rng(2020)
    sizes = [1, 2, 3, 299, 300] + [int(v) for v in rng.integers(1, 301, 195)]
    return [clustered_list(n, rng) for n in sizes] + [DUPLICATES]


def test_matrix_by_hand_duplicates_compensation_and_the_skip_rule():
    d, slots, info = xw.matrix(DUPLICATES, xw.LINEAR, score_thr=0.0)
    # ranks: slot 0, 1, 3, 2.  c = [0, 1, 1, 0.6]; rank 1 and 2: (1 - 1) / (1 - 0) = 0; rank 3: the term of rank 0 alone, 1 - 0.6
    assert info["order"].tolist() == [0, 1, 3, 2] and info["comp"].tolist() == [0.0, 1.0, 1.0, 300.0 / 500.0]
    assert info["scores"].tolist() == [0.75, 0.0, 0.0, 0.25 * (1.0 - 300.0 / 500.0)]
    assert slots.tolist() == [0, 2, 1, 3] and d[:, 4].tolist() == [0.75, 0.25 * (1.0 - 300.0 / 500.0), 0.0, 0.0]
    assert xw.matrix(DUPLICATES, xw.LINEAR, score_thr=0.001)[1].tolist() == [0, 2]
    assert xw.matrix(DUPLICATES, xw.LINEAR, score_thr=0.0, max_out=3)[1].tolist() == [0, 2, 1]
    # compensation: A, B (0.6 with A), C (overlaps B more than A): C's term of B is (1 - r_BC) / (1 - 0.6), larger than 1 - r_BC
    chain = np.array([[10.0, 10.0, 20.0, 20.0, 0.875], [10.0, 15.0, 20.0, 20.0, 0.75], [10.0, 19.0, 20.0, 20.0, 0.625]])
    d, slots, info = xw.matrix(chain, xw.LINEAR, score_thr=0.0)
    r_ac, r_bc = 220.0 / 580.0, 320.0 / 480.0
    assert info["comp"].tolist() == [0.0, 0.6, r_bc]
    assert info["scores"][2] == 0.625 * min((1.0 - r_ac) / 1.0, (1.0 - r_bc) / (1.0 - 0.6)) == 0.625 * (1.0 - r_ac)
    g = xw.matrix(chain, xw.GAUSSIAN, sigma=0.5, score_thr=0.0)[2]["scores"]
    want = 0.625 * np.exp(-max((r_ac * r_ac - 0.0) / 0.5, (r_bc * r_bc - 0.6 * 0.6) / 0.5))
    assert abs(g[2] - want) <= 2 * np.spacing(want) and g[0] == 0.875
    assert xw.matrix(np.zeros((0, 5)), xw.LINEAR)[0].shape == (0, 5)


def test_matrix_equals_the_triple_loop_bit_for_bit_on_200_lists():
    shown = np.zeros(5, bool)
    for k, cand in enumerate(lists_200()):
        for thr, max_out in ((0.05, 0), (0.3, 7)) if k % 20 == 0 else ((0.05, 0),):
            d, slots, info = xw.matrix(cand, xw.LINEAR, score_thr=thr, max_out=max_out)
            nd, nslots = xw.matrix_naive(cand, xw.LINEAR, score_thr=thr, max_out=max_out)
            assert slots.tolist() == nslots.tolist() and d.shape == nd.shape and np.array_equal(d.view(np.uint64), nd.view(np.uint64)), k
            if max_out == 0 and len(cand) >= 50:
                shown |= np.array(xw.matrix_facts(cand, d, slots, info, thr))
        if k % 10 == 0 and cand is not DUPLICATES:      # (the duplicates tie under gaussian) gaussian: math.exp here, numpy's exp there -- the same picks, the scores within two ulps
            d, slots, info = xw.matrix(cand, xw.GAUSSIAN, sigma=0.5, score_thr=0.05)
            nd, nslots = xw.matrix_naive(cand, xw.GAUSSIAN, sigma=0.5, score_thr=0.05)
            assert info["min_gap"] > 1e-9 and slots.tolist() == nslots.tolist(), k
            assert np.array_equal(d[:, :4], nd[:, :4]) and np.all(np.abs(d[:, 4] - nd[:, 4]) <= 2 * np.spacing(nd[:, 4])), k
    assert shown.all(), f"the lists show nothing: facts (a) .. (e) = {shown.tolist()}"


def test_matrix_stays_within_the_derived_bound_of_the_exact_scores_on_200_lists():
    worst, decayed = 0.0, 0
    for k, cand in enumerate(lists_200()):
        assert np.all(cand[:, :4] == np.round(cand[:, :4])) and np.all(np.abs(cand[:, :4]) < 2 ** 20), "the bound's premise: integer boxes"
        d, slots, info = xw.matrix(cand, xw.LINEAR, score_thr=0.0)
        order, escores, bounds = xw.matrix_exact(cand)
        assert order.tolist() == info["order"].tolist()
        for j in range(len(cand)):
            got = Fraction(float(info["scores"][j]))
            assert abs(got - escores[j]) <= Fraction(bounds[j]) * escores[j], (k, j, float(got), float(escores[j]), bounds[j] * 2.0 ** 53)
            decayed += bounds[j] > 0
        worst = max([worst] + bounds)
    # every decayed score is a few roundings: a term's bound is r / (1 - r) + c / (1 - c) + 4 units of 2^-53, and on these
    # integer boxes of sides up to 48 an overlap below 1 is at most 1 - 1 / (2 * 48 * 48)
    assert decayed > 1000 and 0 < worst < 2 * (2 * 2 * 48 * 48 + 4) * 2.0 ** -53
