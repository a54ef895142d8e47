"""Seq-NMS over the candidate lists of a clip's frames (mscnn_detections_merge_seq_fwd, Net.set_seq_nms) without a GPU: the ABI as a C
compiler sees it, every refusal through the library with pointers nobody may touch and a NULL stream (each is decided before any
launch and names the offending value), the workspace sizes, the sticky Net-level setting on a graph-only net and its mutual exclusions
with Soft-NMS, Matrix NMS and weighted boxes fusion, the driver flags, the documents, a case worked by hand, and the witnesses of
tests/seq_witness.py against each other: the float loop against the same loop in exact rationals and against a brute force over every
linked path, and the six facts on the clips the GPU tests ship."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import seq_cases as sc
import seq_witness as sq
from mscnn_amd import hipapi, net as mnet, zoo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
FAKE = C.c_void_p(0x1000)          # 16-byte aligned, never dereferenced: every call below is refused first


def L():
    return hipapi.lib()


def err():
    return L().mscnn_last_error().decode()


def seq(link_thr=0.5, score_thr=0.001, top_k=300, rescore=1, max_out=0, T=4, K=2, overlap="default", cand=FAKE, cap=300, pack=FAKE, ids=FAKE,
        ws=FAKE, ws_bytes=None, params="default"):
    p = C.byref(hipapi.SeqNmsParams(link_thr, score_thr, top_k, rescore, max_out)) if params == "default" else params
    n = max(T * K, 1) if 0 < T * K < 1 << 20 else 1
    ov = (C.c_double * n)(*([0.5] * n)) if overlap == "default" else overlap
    wb = L().mscnn_detections_merge_seq_workspace_bytes(T, K, cap, top_k) if ws_bytes is None else ws_bytes
    return L().mscnn_detections_merge_seq_fwd(ov, p, T, K, cand, cap, pack, ids, ws, C.c_size_t(wb), None)


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_seq_params_mirror_matches_the_header_and_the_entry_points_are_exported():
    text = open(os.path.join(ROOT, "include/mscnn_hip.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\}\s*mscnn_seq_nms_params;", text)
    assert m and [d.strip() for d in m.group(1).split(";") if d.strip()] == ["double link_thr", "double score_thr", "int top_k", "int rescore",
                                                                             "int max_out"]
    assert hipapi.SeqNmsParams._fields_ == [("link_thr", C.c_double), ("score_thr", C.c_double), ("top_k", C.c_int), ("rescore", C.c_int),
                                            ("max_out", C.c_int)]
    assert C.sizeof(hipapi.SeqNmsParams) == 32
    assert [getattr(hipapi.SeqNmsParams, f).offset for f in ("link_thr", "score_thr", "top_k", "rescore", "max_out")] == [0, 8, 16, 20, 24]
    assert re.search(r"MSCNN_SEQ_NMS_AVG = 1, MSCNN_SEQ_NMS_MAX = 2", text) and hipapi.SEQ_NMS_RESCORES == dict(avg=1, max=2)
    for name in ("mscnn_detections_merge_seq_fwd", "mscnn_detections_merge_seq_workspace_bytes"):
        assert hasattr(L(), name), name
    for name in ("mscnn_net_set_seq_nms", "mscnn_net_get_seq_nms", "mscnn_net_detect_merge_sequences"):
        assert hasattr(mnet.lib(), name), name
    assert re.search(r"detections_merge_seq_fwd\s+cand, workspace, pack_dev 16, seq_dev 4: refuses", text), "the op's line of the ALIGNMENT table"
    vp, ci = C.c_void_p, C.c_int
    assert L().mscnn_detections_merge_seq_fwd.argtypes == [vp, vp, ci, ci, vp, ci, vp, vp, vp, C.c_size_t, vp]
    assert L().mscnn_detections_merge_seq_workspace_bytes.argtypes == [ci, ci, ci, ci]
    assert L().mscnn_detections_merge_seq_workspace_bytes.restype == C.c_size_t
    proto = " ".join(re.sub(r"/\*.*?\*/", "", text, flags=re.S).split())
    assert ("int mscnn_detections_merge_seq_fwd(const double* nms_overlap , const mscnn_seq_nms_params* sq, int num_frames, int num_slots, "
            "void* cand, int cand_cap, void* pack_dev, int* seq_dev , void* workspace, size_t workspace_bytes, void* stream);") in proto
    assert "size_t mscnn_detections_merge_seq_workspace_bytes(int num_frames, int num_slots, int cand_cap, int top_k);" in proto
    nett = " ".join(open(os.path.join(ROOT, "include/mscnn_net.h")).read().split())
    assert "int mscnn_net_set_seq_nms(mscnn_net* net, double link_thr, double score_thr, int top_k, int rescore, int max_out);" in nett
    assert "int mscnn_net_detect_merge_sequences(mscnn_net* net, int* seq_host, int cap, const int* seg_dets);" in nett
    assert hasattr(hipapi.Candidates, "merge_seq") and hasattr(mnet.Net, "set_seq_nms") and hasattr(mnet.Net, "detect_merge_sequences")


def test_seq_struct_layout_as_a_c_compiler_sees_it(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or "/opt/rocm/bin/hipcc"      # (the project does not build without hipcc)
    assert shutil.which(cc) or os.path.exists(cc), "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "mscnn_hip.h"\n#include "mscnn_net.h"\n'
                   "_Static_assert(sizeof(mscnn_seq_nms_params) == 32, \"size\");\n"
                   "_Static_assert(offsetof(mscnn_seq_nms_params, link_thr) == 0 && offsetof(mscnn_seq_nms_params, score_thr) == 8 && "
                   "offsetof(mscnn_seq_nms_params, top_k) == 16 && offsetof(mscnn_seq_nms_params, rescore) == 20 && "
                   "offsetof(mscnn_seq_nms_params, max_out) == 24, \"offsets\");\n"
                   "_Static_assert(MSCNN_SEQ_NMS_AVG == 1 && MSCNN_SEQ_NMS_MAX == 2, \"rescore\");\n"
                   "_Static_assert(sizeof(mscnn_wbf_params) == 24 && sizeof(mscnn_soft_nms_params) == 32, \"the neighbours keep their size\");\n")
    r = subprocess.run([cc, "-x", "c", "-std=c11", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_seq_refusals_name_the_value():
    assert seq(params=None) != 0 and "detections_merge_seq: null pointer" in err()
    for which in ("overlap", "cand", "pack", "ws"):
        assert seq(**{which: None}) != 0 and "detections_merge_seq: null pointer" in err(), which
    assert seq(ids=None, cand=C.c_void_p(0x1008)) != 0 and "cand must be 16-byte aligned" in err(), "seq_dev may be NULL"
    for T in (0, -3, 257, 1000):
        assert seq(T=T, ws_bytes=1 << 20) == 1 and f"detections_merge_seq: num_frames {T} is outside [1, 256]" in err()
    for K in (0, -2):
        assert seq(K=K, ws_bytes=1 << 20) == 1 and f"detections_merge_seq: num_slots {K}" in err()
    assert seq(cap=0, ws_bytes=1 << 20) == 1 and "detections_merge_seq: cand_cap 0" in err()
    assert seq(cap=-7, ws_bytes=1 << 20) == 1 and "cand_cap -7" in err()
    assert seq(T=256, K=1 << 10, cap=1 << 16, ws_bytes=1 << 20) == 1 and f"256 frames x {1 << 10} slots x {1 << 16} candidate slots is past 2^31 - 1" in err()
    assert seq(T=256, K=1 << 24, cap=1, ws_bytes=1 << 20) == 1 and "is past 2^31 - 1" in err()
    assert seq(T=1, K=1, cap=(1 << 30) + 1, ws_bytes=1 << 20) == 1 and f"cand_cap {(1 << 30) + 1} is past the sort's 2^30 keys" in err()
    for top_k in (0, -1, 1025, 1 << 20):
        assert seq(top_k=top_k, ws_bytes=1 << 20) == 1 and f"detections_merge_seq: top_k {top_k} is outside [1, 1024]" in err()
    for rescore in (0, 3, -1):
        assert seq(rescore=rescore) == 1 and f"detections_merge_seq: rescore {rescore} is neither 1 (avg) nor 2 (max)" in err()
    for max_out in (-1, -300):
        assert seq(max_out=max_out) == 1 and f"detections_merge_seq: max_out {max_out}" in err()
    for s in (0, 7):
        ov = (C.c_double * 8)(*([0.5] * 8))
        ov[s] = NAN
        assert seq(overlap=ov) == 1 and f"detections_merge_seq: segment {s}: nms_overlap is NaN" in err()
    for which, name in (("cand", "cand"), ("ws", "workspace"), ("pack", "pack_dev")):
        assert seq(**{which: C.c_void_p(0x1008)}) == 1 and f"detections_merge_seq: {name} must be 16-byte aligned" in err(), which
    assert seq(ids=C.c_void_p(0x1002)) == 1 and "detections_merge_seq: seq_dev must be 4-byte aligned" in err()


@pytest.mark.parametrize("thr,text", [(NAN, "link_thr nan"), (0.0, "link_thr 0 "), (1.0, "link_thr 1 "), (-0.5, "link_thr -0.5"), (1.5, "link_thr 1.5"),
                                      (INF, "link_thr inf")])
def test_seq_refuses_a_link_threshold_that_is_nan_or_outside_0_1(thr, text):
    assert seq(link_thr=thr) == 1
    assert "detections_merge_seq: " + text in err() and "not inside (0, 1)" in err(), err()


@pytest.mark.parametrize("thr,text", [(NAN, "score_thr nan"), (-0.001, "score_thr -0.001"), (INF, "score_thr inf"), (-INF, "score_thr -inf")])
def test_seq_refuses_a_score_threshold_that_is_nan_infinite_or_negative(thr, text):
    assert seq(score_thr=thr) == 1
    assert "detections_merge_seq: " + text in err() and "not a finite value >= 0" in err(), err()


def test_workspace_bytes_are_linear_and_a_short_workspace_is_refused():
    wsb = L().mscnn_detections_merge_seq_workspace_bytes
    for T, K, cap, top_k in ((0, 1, 10, 300), (257, 1, 10, 300), (4, 0, 10, 300), (4, 2, 0, 300), (4, 2, -3, 300), (4, 2, 10, 0), (4, 2, 10, 1025),
                             (256, 1 << 10, 1 << 16, 300), (256, 1 << 24, 1, 300), (1, 1, (1 << 30) + 1, 300)):
        assert wsb(T, K, cap, top_k) == 0, (T, K, cap, top_k)
    for T, K, cap, top_k in ((1, 1, 1, 1), (2, 33, 4032, 1024), (8, 1, 4033, 300), (256, 3, 2000, 1024)):
        assert wsb(T, K, cap, top_k) > 0, (T, K, cap, top_k)
    caps = [1, 2, 100, 1000, 4032, 4033, 5000, 8192, 8193, 20000, 1 << 20]
    for part in ([c for c in caps if c <= 4032], [c for c in caps if c > 4032]):      # (a list above 4032 slots is sorted alone: less room)
        sizes = [wsb(8, 1, c, 300) for c in part]
        assert sizes == sorted(sizes) and len(set(sizes)) >= len(part) - 1, "monotone in cand_cap on either sort path"
    assert wsb(1, 1, 4033, 300) > wsb(1, 1, 4032, 300)
    # linear in num_frames * num_slots * top_k * (top_k / 64 + const): per entered box 8 * ceil(top_k / 64) bytes of link bits and 60 of
    # state (box 32, s and score' 8 each, tag, sequence id and prev 4 each), rounded up to 256 per table; plus the sort's need
    for top_k in (1, 64, 65, 300, 1024):
        wk = (top_k + 63) // 64
        state = wsb(64, 2, 100, top_k) - wsb(32, 2, 100, top_k) - (wsb(64, 2, 100, 1) - wsb(32, 2, 100, 1))
        assert abs(state - 64 * (top_k - 1) * 60 - 64 * 8 * (top_k * wk - 1)) <= 9 * 256, top_k
    assert abs((wsb(16, 2, 100, 300) - wsb(8, 2, 100, 300)) - (wsb(24, 2, 100, 300) - wsb(16, 2, 100, 300))) <= 9 * 256, "linear in num_frames"
    assert wsb(8, 6, 100, 300) == wsb(16, 3, 100, 300), "a function of num_frames * num_slots"
    assert wsb(8, 5, 8000, 300) - wsb(8, 1, 8000, 300) < 4 * 8 * 300 * 110, "a list above 4032 slots is sorted alone"
    need = wsb(4, 2, 8000, 300)
    assert seq(cap=8000, ws_bytes=need - 1) == 3, "MSCNN_ERR_WORKSPACE"
    assert f"detections_merge_seq: workspace {need - 1} < {need}" in err()
    assert seq(cap=300, ws_bytes=0) == 3 and "workspace 0 <" in err()


# ---- the Net-level setting on a graph-only net ---------------------------------------------------------------------------------------------------
def graph_net():
    return mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=96, width=320), device=-1)


def test_net_seq_nms_is_off_by_default_sticky_and_unchanged_by_a_refused_value():
    n = graph_net()
    assert n.get_seq_nms() is None
    n.set_seq_nms(0.6, score_thr=0.01, top_k=200, rescore="max", max_out=100)
    want = dict(link_thr=0.6, score_thr=0.01, top_k=200, rescore="max", max_out=100)
    assert n.get_seq_nms() == want
    n.set_nms(type="max")                                    # (other sticky settings do not touch this one)
    n.set_box_voting(0.4)                                    # (the vote runs behind Seq-NMS: no conflict)
    assert n.get_seq_nms() == want and n.get_box_voting() == 0.4 and n.get_soft_nms() is None and n.get_matrix_nms() is None and n.get_wbf() is None
    n.set_box_voting(None)
    bad = [(dict(link_thr=1.0), "link_thr 1 "), (dict(link_thr=-0.1), "link_thr -0.1"), (dict(link_thr=NAN), "link_thr nan"),
           (dict(link_thr=0.5, score_thr=-0.5), "score_thr -0.5"), (dict(link_thr=0.5, score_thr=NAN), "score_thr nan"),
           (dict(link_thr=0.5, score_thr=INF), "score_thr inf"), (dict(link_thr=0.5, top_k=0), "top_k 0 "), (dict(link_thr=0.5, top_k=1025), "top_k 1025 "),
           (dict(link_thr=0.5, rescore=3), "rescore 3 "), (dict(link_thr=0.5, rescore=0), "rescore 0 "), (dict(link_thr=0.5, max_out=-1), "max_out -1"),
           (dict(link_thr=None, max_out=-1), "max_out -1")]
    for kw, text in bad:
        with pytest.raises(mnet.NetError, match="set_seq_nms: " + re.escape(text)):
            n.set_seq_nms(**kw)
        assert n.get_seq_nms() == want, kw
    with pytest.raises(mnet.NetError, match="set_seq_nms: rescore 'median'"):
        n.set_seq_nms(0.5, rescore="median")
    assert n.get_seq_nms() == want
    n.set_seq_nms(0.55)
    assert n.get_seq_nms() == dict(link_thr=0.55, score_thr=0.001, top_k=300, rescore="avg", max_out=0)
    n.set_seq_nms(None)
    assert n.get_seq_nms() is None
    n.set_seq_nms(0.0)
    assert n.get_seq_nms() is None
    lt, st, tk, rs, mo = C.c_double(-1.0), C.c_double(-1.0), C.c_int(-1), C.c_int(-1), C.c_int(-1)
    lib = mnet.lib()
    assert lib.mscnn_net_get_seq_nms(n._h, C.byref(lt), C.byref(st), C.byref(tk), C.byref(rs), C.byref(mo)) == 0 and lt.value == 0.0
    assert (st.value, tk.value, rs.value, mo.value) == (0.001, 300, 1, 0), "the round trip of an off setting keeps the other values"
    assert lib.mscnn_net_get_seq_nms(n._h, None, C.byref(st), C.byref(tk), C.byref(rs), C.byref(mo)) != 0
    with pytest.raises(mnet.NetError, match="detect_merge_sequences: the last mscnn_net_detect_merge_end did not run Seq-NMS"):
        n.detect_merge_sequences()
    # while the setting is on, a clip of more than 256 frames is refused at _begin, naming the value (before the device is asked for)
    n.set_seq_nms(0.5)
    with pytest.raises(mnet.NetError, match=r"detect_merge_begin: num_frames 257 is outside \[1, 256\] while Seq-NMS is on \(set_seq_nms link_thr 0.5\)"):
        n.detect_merge_begin(257, 1, 10)
    with pytest.raises(mnet.NetError, match="graph only"):      # 256 frames pass that check and stop at the next one
        n.detect_merge_begin(256, 1, 10)
    n.set_seq_nms(None)
    with pytest.raises(mnet.NetError, match="graph only"):
        n.detect_merge_begin(257, 1, 10)


def test_seq_nms_excludes_soft_nms_matrix_nms_and_wbf_in_both_orders():
    n = graph_net()
    partners = [("set_soft_nms", lambda: n.set_soft_nms("gaussian"), lambda: n.set_soft_nms(None), n.get_soft_nms,
                 r"set_soft_nms: method 2 while Seq-NMS is on \(set_seq_nms link_thr 0.6\)",
                 r"set_seq_nms: link_thr 0.5 while Soft-NMS is on \(set_soft_nms method 2\)"),
                ("set_matrix_nms", lambda: n.set_matrix_nms("linear"), lambda: n.set_matrix_nms(None), n.get_matrix_nms,
                 r"set_matrix_nms: method 1 while Seq-NMS is on \(set_seq_nms link_thr 0.6\)",
                 r"set_seq_nms: link_thr 0.5 while Matrix NMS is on \(set_matrix_nms method 1\)"),
                ("set_wbf", lambda: n.set_wbf(0.4), lambda: n.set_wbf(None), n.get_wbf,
                 r"set_wbf: thr 0.4 while Seq-NMS is on \(set_seq_nms link_thr 0.6\)",
                 r"set_seq_nms: link_thr 0.5 while weighted boxes fusion is on \(set_wbf thr 0.4\)")]
    for name, on, off, get, refused_partner, refused_seq in partners:
        n.set_seq_nms(0.6, max_out=9)
        with pytest.raises(mnet.NetError, match=refused_partner):
            on()
        assert get() is None and n.get_seq_nms() == dict(link_thr=0.6, score_thr=0.001, top_k=300, rescore="avg", max_out=9), name
        off()                                                # (turning the other one OFF is no conflict)
        n.set_seq_nms(None)
        on()
        kept = get()
        with pytest.raises(mnet.NetError, match=refused_seq):
            n.set_seq_nms(0.5)
        assert n.get_seq_nms() is None and get() == kept and kept is not None, name
        n.set_seq_nms(None)                                  # (off while the other is on: no conflict)
        off()
        n.set_seq_nms(0.5)
        assert n.get_seq_nms()["link_thr"] == 0.5
        n.set_seq_nms(None)


def test_driver_seq_flags_parse(capsys):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import run_cascademscnn
        import run_mscnn_detection
    finally:
        sys.path.pop(0)
    for mod, model in ((run_mscnn_detection, "caltech/mscnn-7s-480"), (run_cascademscnn, "kitti_car/cascade-mscnn-7s-576-2x")):
        base = ["--model", model, "--synthetic", "1"]
        a = mod.parse_args(base)
        assert a.seq_nms is None and a.clip == 8 and a.seq_link == 0.5 and a.seq_top_k == 300 and a.tubelets_out is None
        assert mod.parse_args(base + ["--seq-nms"]).seq_nms == "avg"
        assert mod.parse_args(base + ["--seq-nms", "max"]).seq_nms == "max"
        a = mod.parse_args(base + ["--seq-nms", "avg", "--clip", "3", "--seq-link", "0.4", "--seq-top-k", "100", "--soft-thr", "0.05", "--max-dets", "50",
                                   "--batch", "3", "--tubelets-out", "tubes", "--flip"])
        assert (a.seq_nms, a.clip, a.seq_link, a.seq_top_k, a.soft_thr, a.max_dets, a.batch, a.tubelets_out, a.flip) == \
            ("avg", 3, 0.4, 100, 0.05, 50, 3, "tubes", True)
        assert mod.parse_args(base + ["--seq-nms", "--vote"]).vote == 0.5, "the vote runs behind Seq-NMS"
        for bad in (["--seq-nms", "median"], ["--seq-nms", "--soft-nms", "linear"], ["--seq-nms", "--matrix-nms", "gaussian"], ["--seq-nms", "--wbf"],
                    ["--seq-nms", "--clip", "0"], ["--seq-nms", "--clip", "257"], ["--seq-nms", "--seq-link", "0"], ["--seq-nms", "--seq-link", "1"],
                    ["--seq-nms", "--seq-link", "nan"], ["--seq-nms", "--seq-top-k", "0"], ["--seq-nms", "--seq-top-k", "1025"],
                    ["--seq-nms", "--max-dets", "-1"], ["--seq-nms", "--soft-thr", "-1"], ["--clip", "4"], ["--seq-link", "0.4"], ["--seq-top-k", "10"],
                    ["--tubelets-out", "tubes"]):
            with pytest.raises(SystemExit):
                mod.parse_args(base + bad)
    capsys.readouterr()


def test_docs_describe_seq_nms_and_say_that_it_is_unpinned():
    for doc in ("include/mscnn_hip.h", "include/mscnn_net.h", "DESIGN.md", "INTEGRATION.md", "README.md"):
        text = " ".join(open(os.path.join(ROOT, doc)).read().split())
        assert re.search(r"Seq-NMS", text) and re.search(r"set_seq_nms|merge_seq", text), doc
        at = [m.start() for m in re.finditer(r"Seq-NMS", text)]
        near = lambda pat: any(re.search(pat, text[max(0, a - 2500):a + 7000], re.I) for a in at)      # noqa: E731
        assert near(r"no pin on the reference"), doc
        assert near(r"not evaluated"), doc
    assert "max_out cuts the OUTPUT only" in " ".join(open(os.path.join(ROOT, "include/mscnn_hip.h")).read().replace(" * ", " ").split())
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--seq-nms" in readme and "profiles/detect_merge_seq.txt" in readme
    assert "Seq-NMS" in open(os.path.join(ROOT, "PAPERS.md")).read()


# ---- a case worked by hand ------------------------------------------------------------------------------------------------------------------------
# Three frames, integer boxes, probs exact in float32, link_thr 0.5, nms_overlap 0.3.
HAND = [np.array([[10.0, 10.0, 20.0, 20.0, 0.5],        # A0
                  [100.0, 10.0, 20.0, 20.0, 0.75]]),    # B0: overlaps nothing in any frame
        np.array([[12.0, 10.0, 20.0, 20.0, 0.25]]),     # A1: 360 / 440 with A0
        np.array([[15.0, 10.0, 20.0, 20.0, 0.125],      # C2: 340 / 460 with A1; 380 / 420 with A2 -> suppressed by it
                  [14.0, 10.0, 20.0, 20.0, 0.875]])]    # A2: 360 / 440 with A1


def test_seq_nms_by_hand_three_frames_five_boxes():
    for rescore, sc_path in ((sq.AVG, (0.5 + 0.25 + 0.875) / 3.0), (sq.MAX, 0.875)):
        rows, tr = sq.seq_nms(HAND, 0.5, [0.3] * 3, 0.0625, 300, rescore)
        # sorted positions: frame 0 = [B0, A0], frame 2 = [A2, C2].  V(A2) = 0.5 + 0.25 + 0.875 beats V(B0) = 0.75
        assert tr["paths"] == [[(0, 1), (1, 0), (2, 0)], [(0, 0)]] and tr["suppressed"] == [(2, 1)]
        (d0, s0, q0), (d1, s1, q1), (d2, s2, q2) = rows
        first = [(sc_path, 0, 0), (0.75, 1, 1)]              # (score', slot, seq) of frame 0's rows, in descending score'
        first.sort(key=lambda v: -v[0])
        assert d0[:, 4].tolist() == [v[0] for v in first] and s0.tolist() == [v[1] for v in first] and q0.tolist() == [v[2] for v in first]
        assert d1.tolist() == [[12.0, 10.0, 20.0, 20.0, sc_path]] and q1.tolist() == [0]
        assert d2.tolist() == [[14.0, 10.0, 20.0, 20.0, sc_path]] and s2.tolist() == [1] and q2.tolist() == [0], "C2 never comes out"
    # score_thr keeps C2 out from the start; top_k 1 keeps A0 out of frame 0: A1 then starts the path
    rows, tr = sq.seq_nms(HAND, 0.5, [0.3] * 3, 0.2, 300)
    assert [len(e[0]) for e in tr["ent"]] == [2, 1, 1] and tr["suppressed"] == []
    rows, tr = sq.seq_nms(HAND, 0.5, [0.3] * 3, 0.0, 1)
    assert tr["paths"] == [[(1, 0), (2, 0)], [(0, 0)]] and rows[0][0][:, 4].tolist() == [0.75]
    # max_out cuts the output only
    rows1, tr1 = sq.seq_nms(HAND, 0.5, [0.3] * 3, 0.0625, 300, sq.AVG, max_out=1)
    assert [len(r[0]) for r in rows1] == [1, 1, 1] and tr1["paths"] == [[(0, 1), (1, 0), (2, 0)], [(0, 0)]] and rows1[0][2].tolist() == [1]
    # an overflowed list is an empty frame: nothing links across it
    rows, tr = sq.seq_nms([HAND[0], None, HAND[2]], 0.5, [0.3] * 3, 0.0625, 300)
    assert all(len(p) == 1 for p in tr["paths"]) and len(rows[1][0]) == 0
    assert sq.seq_nms([np.zeros((0, 5))], 0.5, [0.3])[0][0][0].shape == (0, 5)
    ex = sq.seq_exact(HAND, 0.5, [0.3] * 3, 0.0625, 300)
    assert ex["paths"] == [[(0, 1), (1, 0), (2, 0)], [(0, 0)]] and ex["sums"][0] == sq.Fraction(13, 8) and ex["ties"] == 0


# ---- the witnesses against each other ---------------------------------------------------------------------------------------------------------
def tiny_chain(rng, T):
    """T <= 4 frames of 1 .. 5 integer boxes around two spots a few pixels apart, float32 probs: many links, several predecessors."""
    frames = []
    for t in range(T):
        n = int(rng.integers(1, 6))
        spot = rng.integers(0, 2, n)
        xy = np.stack([100 + 60 * spot, np.full(n, 100)], 1) + rng.integers(-5, 6, (n, 2))
        frames.append(np.concatenate([xy, np.full((n, 2), 32.0), rng.uniform(0.05, 1, (n, 1)).astype(np.float32)], 1).astype(np.float64))
    return frames


def test_the_dp_picks_a_maximum_sum_path_of_every_linked_path_on_300_tiny_chains():
    rng = np.random.default_rng(2016)
    iterations = branching = 0
    for k in range(300):
        T = int(rng.integers(1, 5))
        cands = tiny_chain(rng, T)
        ov = [float(v) for v in rng.choice([0.3, 0.5, 0.7], T)]
        ex = sq.seq_exact(cands, 0.5, ov, 0.1, 5)
        for live, total in zip(ex["lives"], ex["sums"]):
            assert total == sq.brute_best(ex["scores"], ex["links"], live), k
            iterations += 1
        rows, tr = sq.seq_nms(cands, 0.5, ov, 0.1, 5)
        if ex["ties"] == 0 and ex["min_gap"] > 2.0 ** -40:
            assert tr["paths"] == ex["paths"], k
        branching += bool(tr["fact6"])
        # every entered box is out exactly once or suppressed; a sequence id is one path
        for t in range(T):
            assert np.all((tr["oq"][t] >= 0) ^ np.isin(np.arange(len(tr["oq"][t])), [j for tt, j in tr["suppressed"] if tt == t]))
    assert iterations > 600 and branching >= 5, "no chain where the argmax over the predecessors is not the lowest index"


@pytest.mark.parametrize("name", list(sc.CLIPS))
def test_the_shipped_clips_show_facts_1_to_6_and_no_pick_of_theirs_was_decided_by_rounding(name):
    classes, passes, lists, T = sc.clip(name)
    K = len(classes)
    assert sc.facts_of(lists, T, score_thr=0.05) == (True,) * 6
    for k in range(K):
        cands = sc.chain_cands(lists, K, k)
        assert sq.seq_facts(cands, sc.LINK, [0.3] * T, 0.05, 300) == (True,) * 6, (name, k)
        rows, tr = sq.seq_nms(cands, sc.LINK, [0.3] * T, 0.05, 300)
        ex = sq.seq_exact(cands, sc.LINK, [0.3] * T, 0.05, 300)
        assert ex["ties"] == 0 and ex["min_gap"] > 2.0 ** -30, "a pick within rounding of its runner-up: the case is not robust"
        assert tr["paths"] == ex["paths"]
        for p, total in zip(tr["paths"], ex["sums"]):       # the float sum, one rounded add per frame, against the exact one
            v = 0.0
            for i, (t, j) in enumerate(p):
                v = tr["ent"][t][1][j] if i == 0 else v + tr["ent"][t][1][j]
            assert abs(sq.Fraction(float(v)) - total) <= total * len(p) * sq.Fraction(1, 2 ** 53)
