"""Weighted boxes fusion over the merged candidates (mscnn_detections_merge_wbf_fwd, Net.set_wbf) without a GPU: the ABI as a C
compiler sees it, every refusal through the library with pointers nobody may touch and a NULL stream (each is decided before any
launch and names the offending value), the workspace sizes, the sticky Net-level setting on a graph-only net and its mutual
exclusions with Soft-NMS, Matrix NMS and box voting, the driver flags, the documents, a case worked by hand, and the witnesses of
tests/wbf_witness.py against each other.

The bound of the float witness's fused coordinates against the exact ones is derived in wbf_witness.wbf_exact, not tuned."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import wbf_witness as ww
from mscnn_amd import hipapi, net as mnet, zoo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
FAKE = C.c_void_p(0x1000)          # 16-byte aligned, never dereferenced: every call below is refused first


def L():
    return hipapi.lib()


def err():
    return L().mscnn_last_error().decode()


def wbf(thr=0.55, skip_thr=0.0, conf_type=1, max_out=0, expected="default", S=4, cand=FAKE, cap=300, pack=FAKE, members=FAKE, ws=FAKE,
        ws_bytes=None, params="default"):
    p = C.byref(hipapi.WbfParams(thr, skip_thr, conf_type, max_out)) if params == "default" else params
    ex = (C.c_int * max(S, 1))(*([1] * max(S, 1))) if expected == "default" else expected
    wb = L().mscnn_detections_merge_wbf_workspace_bytes(S, cap) if ws_bytes is None else ws_bytes
    return L().mscnn_detections_merge_wbf_fwd(p, ex, S, cand, cap, pack, members, ws, C.c_size_t(wb), None)


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_wbf_params_mirror_matches_the_header_and_the_entry_points_are_exported():
    text = open(os.path.join(ROOT, "include/mscnn_hip.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\}\s*mscnn_wbf_params;", text)
    assert m and [d.strip() for d in m.group(1).split(";") if d.strip()] == ["double thr", "double skip_thr", "int conf_type", "int max_out"]
    assert hipapi.WbfParams._fields_ == [("thr", C.c_double), ("skip_thr", C.c_double), ("conf_type", C.c_int), ("max_out", C.c_int)]
    assert C.sizeof(hipapi.WbfParams) == 24
    assert [getattr(hipapi.WbfParams, f).offset for f in ("thr", "skip_thr", "conf_type", "max_out")] == [0, 8, 16, 20]
    assert re.search(r"MSCNN_WBF_CONF_AVG = 1, MSCNN_WBF_CONF_MAX = 2", text) and hipapi.WBF_CONF_TYPES == dict(avg=1, max=2)
    for name in ("mscnn_detections_merge_wbf_fwd", "mscnn_detections_merge_wbf_workspace_bytes"):
        assert hasattr(L(), name), name
    for name in ("mscnn_net_set_wbf", "mscnn_net_get_wbf", "mscnn_net_detect_merge_members"):
        assert hasattr(mnet.lib(), name), name
    assert re.search(r"detections_merge_wbf_fwd\s+cand, workspace, pack_dev 16, members_dev 4: refuses", text), "the op's line of the ALIGNMENT table"
    vp, ci = C.c_void_p, C.c_int
    assert L().mscnn_detections_merge_wbf_fwd.argtypes == [vp, vp, ci, vp, ci, vp, vp, vp, C.c_size_t, vp]
    assert L().mscnn_detections_merge_wbf_workspace_bytes.argtypes == [ci, ci]
    assert L().mscnn_detections_merge_wbf_workspace_bytes.restype == C.c_size_t
    proto = " ".join(re.sub(r"/\*.*?\*/", "", text, flags=re.S).split())
    assert ("int mscnn_detections_merge_wbf_fwd(const mscnn_wbf_params* wbf, const int* expected , int num_segments, void* cand, "
            "int cand_cap, void* pack_dev, int* members_dev , void* workspace, size_t workspace_bytes, void* stream);") in proto
    assert "size_t mscnn_detections_merge_wbf_workspace_bytes(int num_segments, int cand_cap);" in proto
    assert hasattr(hipapi.Candidates, "merge_wbf") and hasattr(mnet.Net, "set_wbf") and hasattr(mnet.Net, "detect_merge_members")


def test_wbf_struct_layout_as_a_c_compiler_sees_it(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or "/opt/rocm/bin/hipcc"      # (the project does not build without hipcc)
    assert shutil.which(cc) or os.path.exists(cc), "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "mscnn_hip.h"\n#include "mscnn_net.h"\n'
                   "_Static_assert(sizeof(mscnn_wbf_params) == 24, \"size\");\n"
                   "_Static_assert(offsetof(mscnn_wbf_params, thr) == 0 && offsetof(mscnn_wbf_params, skip_thr) == 8 && "
                   "offsetof(mscnn_wbf_params, conf_type) == 16 && offsetof(mscnn_wbf_params, max_out) == 20, \"offsets\");\n"
                   "_Static_assert(MSCNN_WBF_CONF_AVG == 1 && MSCNN_WBF_CONF_MAX == 2, \"conf types\");\n"
                   "_Static_assert(sizeof(mscnn_soft_nms_params) == 32 && sizeof(mscnn_matrix_nms_params) == 32, \"the neighbours keep their size\");\n")
    r = subprocess.run([cc, "-x", "c", "-std=c11", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_wbf_refusals_name_the_value():
    assert wbf(params=None) != 0 and "detections_merge_wbf: null pointer" in err()
    for which in ("expected", "cand", "pack", "ws"):
        assert wbf(**{which: None}) != 0 and "detections_merge_wbf: null pointer" in err(), which
    assert wbf(members=None, cand=C.c_void_p(0x1008)) != 0 and "cand must be 16-byte aligned" in err(), "members_dev may be NULL"
    assert wbf(S=0, ws_bytes=1 << 20) != 0 and "detections_merge_wbf: 0 segments" in err()
    assert wbf(S=-2, ws_bytes=1 << 20) != 0 and "-2 segments" in err()
    assert wbf(cap=0, ws_bytes=1 << 20) != 0 and "detections_merge_wbf: cand_cap 0" in err()
    assert wbf(cap=-7, ws_bytes=1 << 20) != 0 and "cand_cap -7" in err()
    assert wbf(S=1 << 16, cap=1 << 16, ws_bytes=1 << 20) != 0 and f"{1 << 16} segments x {1 << 16} slots is past 2^31 - 1" in err()
    assert wbf(S=1, cap=(1 << 30) + 1, ws_bytes=1 << 20) != 0 and f"cand_cap {(1 << 30) + 1} is past the sort's 2^30 keys" in err()
    for conf_type in (0, 3, -1):
        assert wbf(conf_type=conf_type) != 0 and f"detections_merge_wbf: conf_type {conf_type} is neither 1 (avg) nor 2 (max)" in err()
    for max_out in (-1, -300):
        assert wbf(max_out=max_out) != 0 and f"detections_merge_wbf: max_out {max_out}" in err()
    for s, v in ((0, 0), (3, -2)):
        ex = (C.c_int * 4)(1, 2, 3, 4)
        ex[s] = v
        assert wbf(expected=ex) != 0 and f"detections_merge_wbf: segment {s}: expected {v}" in err()
    for which, name in (("cand", "cand"), ("ws", "workspace"), ("pack", "pack_dev")):
        assert wbf(**{which: C.c_void_p(0x1008)}) != 0 and f"detections_merge_wbf: {name} must be 16-byte aligned" in err(), which
    assert wbf(members=C.c_void_p(0x1002)) != 0 and "detections_merge_wbf: members_dev must be 4-byte aligned" in err()


@pytest.mark.parametrize("thr,text", [(NAN, "thr nan"), (0.0, "thr 0 "), (1.0, "thr 1 "), (-0.5, "thr -0.5"), (1.5, "thr 1.5"), (INF, "thr inf")])
def test_wbf_refuses_a_threshold_that_is_nan_or_outside_0_1(thr, text):
    assert wbf(thr=thr) != 0
    assert "detections_merge_wbf: " + text in err() and "not inside (0, 1)" in err(), err()


@pytest.mark.parametrize("skip,text", [(NAN, "skip_thr nan"), (-0.001, "skip_thr -0.001"), (INF, "skip_thr inf"), (-INF, "skip_thr -inf")])
def test_wbf_refuses_a_skip_threshold_that_is_nan_infinite_or_negative(skip, text):
    assert wbf(skip_thr=skip) != 0
    assert "detections_merge_wbf: " + text in err() and "not a finite value >= 0" in err(), err()


def test_workspace_bytes_are_linear_and_a_short_workspace_is_refused():
    wsb = L().mscnn_detections_merge_wbf_workspace_bytes
    for S, cap in ((0, 10), (-1, 10), (4, 0), (4, -3), (1 << 16, 1 << 16), (1, (1 << 30) + 1)):
        assert wsb(S, cap) == 0, (S, cap)
    for S, cap in ((1, 1), (33, 4032), (1, 4033), (1, 8000), (3, 20000)):
        assert wsb(S, cap) > 0, (S, cap)
    caps = [1, 2, 100, 255, 256, 257, 1000, 4032, 4033, 4096, 4097, 5000, 8192, 8193, 20000, 40000, 1 << 20]
    sizes = [wsb(1, c) for c in caps]
    assert sizes == sorted(sizes) and len(set(sizes)) > 10, "monotone in cand_cap"
    # linear.  Per slot of a list: the sorted slice (32 + 8 + 4 bytes), the keys of the sort's power of two above 4032 slots (at most
    # 2 x 8), and the walk's areas: five running sums (40), the fused box (32), conf (8), members and first (2 x 4) -- 148 bytes
    assert wsb(1, 20000) < 150 * 20000 + wsb(1, 1)
    assert wsb(1, 40000) < 2 * wsb(1, 20000) + 4096 and wsb(1, 1 << 20) < 150 * (1 << 20) + wsb(1, 1)
    assert wsb(33, 300) > wsb(32, 300) > wsb(1, 300) and wsb(5, 8000) == wsb(1, 8000), "a list above 4032 slots is served alone"
    need = wsb(4, 8000)
    assert wbf(cap=8000, ws_bytes=need - 1) == 3, "MSCNN_ERR_WORKSPACE"
    assert f"detections_merge_wbf: workspace {need - 1} < {need}" in err()
    assert wbf(cap=300, ws_bytes=0) == 3 and "workspace 0 <" in err()


# ---- the Net-level setting on a graph-only net ---------------------------------------------------------------------------------------------------
def graph_net():
    return mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=96, width=320), device=-1)


def test_net_wbf_is_off_by_default_sticky_and_unchanged_by_a_refused_value():
    n = graph_net()
    assert n.get_wbf() is None
    n.set_wbf(0.6, skip_thr=0.01, conf="max", expected=3, max_out=100)
    want = dict(thr=0.6, skip_thr=0.01, conf="max", expected=3, max_out=100)
    assert n.get_wbf() == want
    n.set_nms(type="max")                                    # (other sticky settings do not touch this one)
    assert n.get_wbf() == want and n.get_box_voting() is None and n.get_soft_nms() is None and n.get_matrix_nms() is None
    bad = [(dict(thr=1.0), "thr 1 "), (dict(thr=-0.1), "thr -0.1"), (dict(thr=NAN), "thr nan"), (dict(thr=0.5, skip_thr=-0.5), "skip_thr -0.5"),
           (dict(thr=0.5, skip_thr=NAN), "skip_thr nan"), (dict(thr=0.5, skip_thr=INF), "skip_thr inf"), (dict(thr=0.5, conf=3), "conf_type 3 "),
           (dict(thr=0.5, conf=0), "conf_type 0 "), (dict(thr=0.5, expected=-1), "expected -1"), (dict(thr=0.5, max_out=-1), "max_out -1"),
           (dict(thr=None, max_out=-1), "max_out -1")]
    for kw, text in bad:
        with pytest.raises(mnet.NetError, match="set_wbf: " + re.escape(text)):
            n.set_wbf(**kw)
        assert n.get_wbf() == want, kw
    with pytest.raises(mnet.NetError, match="set_wbf: conf 'median'"):
        n.set_wbf(0.5, conf="median")
    assert n.get_wbf() == want
    n.set_wbf(0.55)
    assert n.get_wbf() == dict(thr=0.55, skip_thr=0.0, conf="avg", expected=0, max_out=0)
    n.set_wbf(None)
    assert n.get_wbf() is None
    n.set_wbf(0.0)
    assert n.get_wbf() is None
    th, sk, ct, ex, mo = C.c_double(-1.0), C.c_double(-1.0), C.c_int(-1), C.c_int(-1), C.c_int(-1)
    lib = mnet.lib()
    assert lib.mscnn_net_get_wbf(n._h, C.byref(th), C.byref(sk), C.byref(ct), C.byref(ex), C.byref(mo)) == 0 and th.value == 0.0
    assert lib.mscnn_net_get_wbf(n._h, None, C.byref(sk), C.byref(ct), C.byref(ex), C.byref(mo)) != 0
    with pytest.raises(mnet.NetError, match="detect_merge_members: the last mscnn_net_detect_merge_end did not run weighted boxes fusion"):
        n.detect_merge_members()


def test_wbf_excludes_soft_nms_matrix_nms_and_box_voting_in_both_orders():
    n = graph_net()
    partners = [("set_soft_nms", lambda: n.set_soft_nms("gaussian"), lambda: n.set_soft_nms(None), n.get_soft_nms,
                 r"set_soft_nms: method 2 while weighted boxes fusion is on \(set_wbf thr 0.6\)", r"set_wbf: thr 0.5 while Soft-NMS is on \(set_soft_nms method 2\)"),
                ("set_matrix_nms", lambda: n.set_matrix_nms("linear"), lambda: n.set_matrix_nms(None), n.get_matrix_nms,
                 r"set_matrix_nms: method 1 while weighted boxes fusion is on \(set_wbf thr 0.6\)",
                 r"set_wbf: thr 0.5 while Matrix NMS is on \(set_matrix_nms method 1\)"),
                ("set_box_voting", lambda: n.set_box_voting(0.4), lambda: n.set_box_voting(None), n.get_box_voting,
                 r"set_box_voting: thr 0.4 while weighted boxes fusion is on \(set_wbf thr 0.6\)",
                 r"set_wbf: thr 0.5 while box voting is on \(set_box_voting thr 0.4\)")]
    for name, on, off, get, refused_partner, refused_wbf in partners:
        n.set_wbf(0.6, max_out=9)
        with pytest.raises(mnet.NetError, match=refused_partner):
            on()
        assert get() is None and n.get_wbf() == dict(thr=0.6, skip_thr=0.0, conf="avg", expected=0, max_out=9), name
        off()                                                # (turning the other one OFF is no conflict)
        n.set_wbf(None)
        on()
        kept = get()
        with pytest.raises(mnet.NetError, match=refused_wbf):
            n.set_wbf(0.5)
        assert n.get_wbf() is None and get() == kept and kept is not None, name
        n.set_wbf(None)                                      # (off while the other is on: no conflict)
        off()
        n.set_wbf(0.5)
        assert n.get_wbf()["thr"] == 0.5
        n.set_wbf(None)


def test_driver_wbf_flags_parse(capsys):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import run_cascademscnn
        import run_mscnn_detection
    finally:
        sys.path.pop(0)
    for mod, model in ((run_mscnn_detection, "caltech/mscnn-7s-480"), (run_cascademscnn, "kitti_car/cascade-mscnn-7s-576-2x")):
        base = ["--model", model, "--synthetic", "1"]
        a = mod.parse_args(base)
        assert a.wbf is None and a.wbf_skip == 0.0 and a.wbf_conf == "avg" and a.wbf_expected == 0 and a.max_dets == 0
        assert mod.parse_args(base + ["--wbf"]).wbf == 0.55
        assert mod.parse_args(base + ["--wbf", "0.6"]).wbf == 0.6
        a = mod.parse_args(base + ["--wbf", "0.5", "--wbf-skip", "0.05", "--wbf-conf", "max", "--wbf-expected", "4", "--max-dets", "300", "--flip"])
        assert (a.wbf, a.wbf_skip, a.wbf_conf, a.wbf_expected, a.max_dets, a.flip) == (0.5, 0.05, "max", 4, 300, True)
        assert a.soft_nms is None and a.matrix_nms is None and a.vote is None
        for bad in (["--wbf", "0"], ["--wbf", "1"], ["--wbf", "nan"], ["--wbf", "--soft-nms", "linear"], ["--wbf", "--matrix-nms", "gaussian"],
                    ["--wbf", "--vote"], ["--wbf", "--wbf-skip", "-1"], ["--wbf", "--wbf-skip", "inf"], ["--wbf", "--wbf-conf", "median"],
                    ["--wbf", "--wbf-expected", "-1"], ["--wbf", "--max-dets", "-1"], ["--wbf-skip", "0.1"], ["--wbf-conf", "max"],
                    ["--wbf-expected", "2"], ["--max-dets", "5"], ["--wbf", "--soft-thr", "0.01"], ["--wbf", "--batch", "2"]):
            with pytest.raises(SystemExit):
                mod.parse_args(base + bad)
    capsys.readouterr()


def test_docs_describe_wbf_and_say_that_it_is_unpinned():
    for doc in ("include/mscnn_hip.h", "include/mscnn_net.h", "DESIGN.md", "INTEGRATION.md", "README.md"):
        text = " ".join(open(os.path.join(ROOT, doc)).read().split())
        assert re.search(r"weighted boxes fusion", text, re.I) and re.search(r"set_wbf|merge_wbf", text), doc
        at = [m.start() for m in re.finditer(r"weighted boxes fusion", text, re.I)]
        near = lambda pat: any(re.search(pat, text[max(0, a - 2500):a + 6000], re.I) for a in at)      # noqa: E731
        assert near(r"no pin on the reference"), doc
        assert near(r"not evaluated"), doc
        assert near(r"min\(members, (T|N|expected)\w*(\[s\])?\) / "), doc
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--wbf" in readme and "profiles/detect_merge_wbf.txt" in readme


# ---- a case worked by hand ------------------------------------------------------------------------------------------------------------------------
# 7 integer boxes, probs exact in float32, thr 0.55.  Walk order by prob: slots 0 1 2 3 4 5 6 as listed.
HAND = np.array([[10.0, 10.0, 20.0, 20.0, 0.75],       # opens cluster 0
                 [100.0, 10.0, 20.0, 20.0, 0.625],     # disjoint: opens cluster 1
                 [10.0, 12.0, 20.0, 20.0, 0.5],        # r with cluster 0 = 360 / 440 > 0.55: joins it
                 [200.0, 200.0, 10.0, 10.0, 0.4375],   # disjoint: opens cluster 2
                 [100.0, 14.0, 20.0, 20.0, 0.375],     # r with cluster 1 = 320 / 480 = 2/3: joins it
                 [12.0, 10.0, 20.0, 20.0, 0.25],       # r with the FUSED cluster 0 (below): joins it
                 [300.0, 300.0, 10.0, 10.0, 0.03125]])  # under skip_thr 0.0625: never enters


def test_wbf_by_hand_three_clusters_seven_boxes():
    # cluster 0 after slot 2: sw = 1.25, sy = 0.75 * 10 + 0.5 * 12 = 13.5 -> y = 10.8; x = 10, w = h = 20 (all exact but 13.5 / 1.25)
    f0y = (0.75 * 10.0 + 0.5 * 12.0) / 1.25
    # slot 5 against [10, f0y, 20, 20]: iw = 18, ih = min(f0y + 20, 30) - max(f0y, 10) = 30 - f0y
    ih = 30.0 - f0y
    r5 = (18.0 * ih) / (400.0 + 400.0 - 18.0 * ih)
    assert r5 > 0.55
    sw0 = 1.25 + 0.25
    F0 = [(0.75 * 10 + 0.5 * 10 + 0.25 * 12) / sw0, (13.5 + 0.25 * 10) / sw0, (0.75 * 20 + 0.5 * 20 + 0.25 * 20) / sw0, 20.0]
    F1 = [100.0, (0.625 * 10 + 0.375 * 14) / 1.0, 20.0, 20.0]
    F2 = [200.0, 200.0, 10.0, 10.0]
    for conf_type, c0, c1, c2 in ((ww.AVG, sw0 / 3.0, 1.0 / 2.0, 0.4375), (ww.MAX, 0.75, 0.625, 0.4375)):
        d, first, members, cluster_of, gap = ww.wbf(HAND, 0.55, 0.0625, conf_type, 1)
        assert cluster_of.tolist() == [0, 1, 0, 2, 1, 0, -1]
        assert d.tolist() == [F0 + [c0], F1 + [c1], F2 + [c2]] and first.tolist() == [0, 1, 3] and members.tolist() == [3, 2, 1]
        # expected 3: conf * min(members, 3) / 3 -- cluster 0 keeps its conf, cluster 1 gets 2/3, the singleton 1/3
        d3, first3, members3, _, _ = ww.wbf(HAND, 0.55, 0.0625, conf_type, 3)
        want = [(c0 * 3.0 / 3.0, 0), (c1 * 2.0 / 3.0, 1), (c2 * 1.0 / 3.0, 3)]
        want.sort(key=lambda t: -t[0])
        assert d3[:, 4].tolist() == [w[0] for w in want] and first3.tolist() == [w[1] for w in want]
        assert ww.wbf(HAND, 0.55, 0.0625, conf_type, 3, max_out=2)[1].tolist() == first3[:2].tolist()
    # the singleton's box and a cluster of one's box are bit for bit the candidate's
    assert np.array_equal(ww.wbf(HAND, 0.55, 0.0625, ww.AVG, 1)[0][2, :4], HAND[3, :4])
    assert ww.wbf(np.zeros((0, 5)))[0].shape == (0, 5)
    # the exact walk agrees, and its fused boxes are the hand's fractions
    eco, fused, emem, bounds = ww.wbf_exact(HAND, 0.55, 0.0625)
    assert eco.tolist() == [0, 1, 0, 2, 1, 0, -1] and emem.tolist() == [3, 2, 1] and bounds[2] == 0.0
    assert fused[0][1] == Fraction(16) / Fraction(3, 2) and fused[1][1] == Fraction(23, 2)


# ---- the witnesses against each other ---------------------------------------------------------------------------------------------------------
def clustered_list(n, rng):
    """n integer boxes in about n / 5 clusters a few pixels apart (sides 28 / 32 / 36: most pairs of a cluster overlap by more than
    0.55), coordinates >= 0, float32 probs in [0.05, 1)."""
    m = rng.integers(0, max(1, n // 5), n)
    xy = np.stack([100 + 100 * (m % 8), 100 + 100 * (m // 8)], 1) + rng.integers(-5, 6, (n, 2))
    return np.concatenate([xy, rng.choice([28, 32, 36], (n, 2)), rng.uniform(0.05, 1, (n, 1)).astype(np.float32)], 1).astype(np.float64)


FACTOR = 2.0 ** 20      # min_gap must exceed the coordinates' bound by this: a relative error e of a fused coordinate below 2^10 moves
                        # iw or ih by at most 2^11 e absolutely and r (sides >= 28, so u >= 784) by well under 2^11 e relatively to thr


def test_wbf_agrees_with_the_exact_walk_within_the_derived_bound_on_200_lists():
    rng = np.random.default_rng(2021)
    sizes = [1, 2, 3, 59, 60] + [int(v) for v in rng.integers(1, 61, 195)]
    left_out, fused_clusters, shown, worst = 0, 0, np.zeros(5, bool), 0.0
    for k, n in enumerate(sizes):
        cand = clustered_list(n, rng)
        assert np.all(cand[:, :4] >= 0) and np.all(cand[:, :4] < 2 ** 10) and np.all(cand[:, 4] > 0), "the bound's premise"
        w = ww._walk(cand, 0.55, 0.1)
        d, first, members, cluster_of, gap = ww.wbf(cand, 0.55, 0.1, ww.AVG, 2)
        eco, fused, emem, bounds = ww.wbf_exact(cand, 0.55, 0.1)
        if not gap > FACTOR * max(bounds + [0.0]):
            left_out += 1
            continue
        assert gap > FACTOR * max(bounds + [0.0])
        assert eco.tolist() == cluster_of.tolist() and emem.tolist() == w["members"].tolist(), k
        for c in range(w["C"]):
            for q in range(4):
                got = Fraction(float(w["F"][c, q]))
                assert abs(got - fused[c][q]) <= Fraction(bounds[c]) * fused[c][q], (k, c, q, float(got), float(fused[c][q]), bounds[c] * 2.0 ** 53)
            fused_clusters += bounds[c] > 0
        worst = max([worst] + bounds)
        if n >= 30:
            shown |= np.array(ww.wbf_facts(cand, 0.55, 0.1, ww.AVG, 2))
    assert left_out <= len(sizes) * 5 // 100, f"{left_out} of {len(sizes)} lists have a min_gap under {FACTOR:g} x their bound"
    assert fused_clusters > 500 and 0 < worst <= 2 * 60 * 1.001 * 2.0 ** -53
    assert shown.all(), f"the lists show nothing: facts 1 .. 5 = {shown.tolist()}"
