"""bbNms's knobs on the final stage (mscnn_nms_params) without a GPU: the struct against the headers, the new exports, every refusal
(before any launch, naming the value), NULL = the default struct, the sticky Net setting on a graph-only net, the driver flags, and
the numpy witness of nmsMax (tests/nms_witness.py) against bbNms's own example and the oracle's greedy / union stage."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import nms_witness as wit
from mscnn_amd import hipapi, net as mnet, zoo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def hip_lib():
    return hipapi.lib()      # (loads without a GPU)


def header_fields(header):
    text = open(os.path.join(ROOT, header)).read()
    m = re.search(r"typedef struct \{([^}]*)\}\s*mscnn_nms_params;", text)
    assert m, header
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return [tuple(d.split()) for d in body.split(";") if d.strip()]


@pytest.mark.parametrize("header", ["include/mscnn_hip.h", "include/mscnn_net.h"])
def test_struct_mirrors_match_the_headers(header):
    want = [("int", "type"), ("int", "ovr_dnm"), ("double", "thr"), ("float", "det_thr")]
    assert header_fields(header) == want
    ctype = {"int": C.c_int, "double": C.c_double, "float": C.c_float}
    for S in (hipapi.NmsParams, mnet.NmsParams):
        assert [(n, t) for n, t in S._fields_] == [(n, ctype[t]) for t, n in want]
        assert C.sizeof(S) == 24 and [getattr(S, n).offset for _, n in want] == [0, 4, 8, 16]


def test_struct_layout_as_a_c_compiler_sees_it_with_both_headers(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or "/opt/rocm/bin/hipcc"      # (the project does not build without hipcc)
    assert shutil.which(cc) or os.path.exists(cc), "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "mscnn_net.h"\n#include "mscnn_hip.h"\n#include "mscnn_net.h"\n'
                   "_Static_assert(sizeof(mscnn_nms_params) == 24, \"size\");\n"
                   "_Static_assert(offsetof(mscnn_nms_params, type) == 0 && offsetof(mscnn_nms_params, ovr_dnm) == 4 && "
                   "offsetof(mscnn_nms_params, thr) == 8 && offsetof(mscnn_nms_params, det_thr) == 16, \"offsets\");\n"
                   "_Static_assert(sizeof(mscnn_detections_desc) == 88, \"the existing desc keeps its size\");\n")
    r = subprocess.run([cc, "-x", "c", "-std=c11", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert C.sizeof(hipapi.DetectionsDesc) == 88


def test_new_entry_points_are_exported():
    L = hip_lib()
    for name in ("mscnn_detections_multi_nms_fwd", "mscnn_detections_cascade_multi_nms_fwd", "mscnn_detections_nms_fwd",
                 "mscnn_detections_cascade_nms_fwd", "mscnn_nms_params_resolve", "mscnn_nms_params_from_names"):
        assert hasattr(L, name), name
    N = mnet.lib()
    assert hasattr(N, "mscnn_net_set_nms") and hasattr(N, "mscnn_net_get_nms")


def resolve(p):
    out = hipapi.NmsParams(9, 9, 9.0, 9.0)
    rc = hip_lib().mscnn_nms_params_resolve(None if p is None else C.byref(p), C.byref(out))
    return rc, hip_lib().mscnn_last_error().decode(), bytes(out)


def test_null_and_the_default_struct_resolve_to_the_same_bytes():
    """What a nms pointer contributes to a launch is the resolved struct (mscnn_hip.h): NULL, the all-default struct and bbNms's
    defaults by name give one and the same block, padding included."""
    rc0, _, b0 = resolve(None)
    rc1, _, b1 = resolve(hipapi.NmsParams(0, 0, -INF, 0.0))
    assert rc0 == 0 and rc1 == 0 and b0 == b1 and len(b0) == 24
    assert b0 == bytes(hipapi.nms_params()) == bytes(hipapi.nms_params("maxg", "union", None, 0.0, maxn=INF))
    d = hipapi.NmsParams.from_buffer_copy(b0)
    assert (d.type, d.ovr_dnm, d.thr, d.det_thr) == (0, 0, -INF, 0.0) and b0[20:] == b"\0\0\0\0"
    rc, _, b = resolve(hipapi.NmsParams(1, 1, 0.25, 0.5))
    assert rc == 0 and b != b0 and hipapi.NmsParams.from_buffer_copy(b).thr == 0.25


REFUSED = [
    (hipapi.NmsParams(2, 0, -INF, 0.0), r"type 2 \('ms'\).*nonMaxSuprList"),
    (hipapi.NmsParams(3, 0, -INF, 0.0), r"type 3 \('cover'\).*summation order"),
    (hipapi.NmsParams(4, 0, -INF, 0.0), r"type 4 \('none'\)"),
    (hipapi.NmsParams(7, 0, -INF, 0.0), r"type 7 "),
    (hipapi.NmsParams(-1, 0, -INF, 0.0), r"type -1 "),
    (hipapi.NmsParams(0, 2, -INF, 0.0), r"ovr_dnm 2 "),
    (hipapi.NmsParams(0, 0, float("nan"), 0.0), r"thr is NaN"),
    (hipapi.NmsParams(0, 0, -INF, -0.5), r"det_thr -0.5 "),
    (hipapi.NmsParams(0, 0, -INF, INF), r"det_thr inf "),
]


@pytest.mark.parametrize("k", range(len(REFUSED)))
def test_refused_values_name_themselves_before_any_launch(k):
    """Through the resolver and through all four *_nms_fwd entry points with pointers nobody may touch (0x1000): every call is
    refused first."""
    p, match = REFUSED[k]
    rc, err, _ = resolve(p)
    assert rc != 0 and re.search(match, err), err
    L = hip_lib()
    fake = C.c_void_p(0x1000)
    descs = (hipapi.DetectionsDesc * 4)()
    for d in descs:
        d.ncls, d.cls_id = 3, 2
    outs = (hipapi.CascadeOutput * 1)()
    outs[0].boxes = outs[0].cls_prob = outs[0].props = 0x1000
    outs[0].ncls = 3
    big = C.c_size_t(1 << 40)
    calls = [
        lambda: L.mscnn_detections_multi_nms_fwd(descs, C.byref(p), 2, 2, fake, fake, fake, 100, 60, fake, 200, fake, big, None),
        lambda: L.mscnn_detections_cascade_multi_nms_fwd(descs, C.c_float(0.0), C.byref(p), 2, 1, 2, outs, 100, 60, fake, 200, fake, big, None),
        lambda: L.mscnn_detections_nms_fwd(descs, C.byref(p), fake, fake, fake, 100, fake, fake, fake, fake, big, None),
        lambda: L.mscnn_detections_cascade_nms_fwd(descs, C.c_float(0.0), C.byref(p), fake, fake, fake, 100, fake, fake, fake, fake, big, None),
    ]
    for call in calls:
        assert call() != 0
        assert re.search(match, L.mscnn_last_error().decode()), L.mscnn_last_error().decode()


def test_names_as_in_the_scripts_and_a_finite_maxn():
    p = hipapi.nms_params("max", "min", thr=0.3, det_thr=0.25)
    assert (p.type, p.ovr_dnm, p.thr, p.det_thr) == (1, 1, 0.3, 0.25)
    for kw, match in [(dict(type="ms"), "'ms'"), (dict(type="cover"), "'cover'"), (dict(type="none"), "'none'"),
                      (dict(type="maxx"), "unknown type 'maxx'"), (dict(ovr_dnm="inter"), "unknown ovr_dnm 'inter'"),
                      (dict(maxn=500), "maxn 500"), (dict(maxn=2), "maxn 2")]:
        with pytest.raises(hipapi.MscnnError, match=match):
            hipapi.nms_params(**kw)


def test_cascade_calls_refuse_the_plain_stage_det_thr_and_the_tiled_path_a_non_default_setting():
    L = hip_lib()
    fake, big = C.c_void_p(0x1000), C.c_size_t(1 << 40)
    descs = (hipapi.DetectionsDesc * 4)()
    for d in descs:
        d.ncls, d.cls_id = 3, 2
    outs = (hipapi.CascadeOutput * 1)()
    outs[0].boxes = outs[0].cls_prob = outs[0].props = 0x1000
    outs[0].ncls = 3
    p = hipapi.NmsParams(1, 0, -INF, 0.5)
    assert L.mscnn_detections_cascade_multi_nms_fwd(descs, C.c_float(0.0), C.byref(p), 2, 1, 2, outs, 100, 60, fake, 200, fake, big, None) != 0
    assert "det_thr 0.5 is the plain stage's" in L.mscnn_last_error().decode()
    assert L.mscnn_detections_cascade_nms_fwd(descs, C.c_float(0.0), C.byref(p), fake, fake, fake, 100, fake, fake, fake, fake, big, None) != 0
    assert "det_thr 0.5 is the plain stage's" in L.mscnn_last_error().decode()
    # more rows than the one-workgroup path holds: the tiled kernels have the default setting only -- refused before their first launch
    p = hipapi.NmsParams(1, 1, -INF, 0.0)
    assert L.mscnn_detections_nms_fwd(descs, C.byref(p), fake, fake, fake, 4033, fake, fake, fake, fake, big, None) != 0
    err = L.mscnn_last_error().decode()
    assert "4033 rows > 4032" in err and "type 1" in err and "ovr_dnm 1" in err
    assert L.mscnn_detections_multi_nms_fwd(descs, C.byref(p), 2, 2, fake, fake, fake, 100, 4033, fake, 200, fake, big, None) != 0
    assert "4033 rows per image > 4032" in L.mscnn_last_error().decode()


def test_net_setting_is_sticky_validated_and_readable_without_a_device():
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=96, width=320), device=-1)
    dflt = dict(type="maxg", ovr_dnm="union", thr=None, det_thr=0.0)
    assert n.get_nms() == dflt
    n.set_nms(type="max", ovr_dnm="min", thr=0.125, det_thr=0.5)
    assert n.get_nms() == dict(type="max", ovr_dnm="min", thr=0.125, det_thr=0.5)
    for kw, match in [(dict(type="ms"), "'ms'"), (dict(type="cover"), "'cover'"), (dict(type="none"), "'none'"), (dict(type="best"), "'best'"),
                      (dict(ovr_dnm="area"), "'area'"), (dict(maxn=100), "maxn 100"), (dict(thr=float("nan")), "thr is NaN"),
                      (dict(det_thr=-1.0), "det_thr -1")]:
        with pytest.raises(mnet.NetError, match=match):
            n.set_nms(**kw)
        assert n.get_nms() == dict(type="max", ovr_dnm="min", thr=0.125, det_thr=0.5)      # a refused call changes nothing
    n.set_nms(None)
    assert n.get_nms() == dflt
    n.set_nms(ovr_dnm="min")
    assert n.get_nms() == dict(dflt, ovr_dnm="min")
    n.set_nms()
    assert n.get_nms() == dflt


def test_driver_flags_parse():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import run_cascademscnn
        import run_mscnn_detection
    finally:
        sys.path.pop(0)
    a = run_mscnn_detection.parse_args(["--model", "caltech/mscnn-7s-480", "--synthetic", "1"])
    assert (a.nms_type, a.ovr_dnm, a.nms_thr, a.det_thr) == ("maxg", "union", None, 0.0)
    a = run_mscnn_detection.parse_args(["--model", "caltech/mscnn-7s-480", "--synthetic", "1", "--nms-type", "max", "--ovr-dnm", "min",
                                        "--nms-thr", "0.1", "--det-thr", "0.05"])
    assert (a.nms_type, a.ovr_dnm, a.nms_thr, a.det_thr) == ("max", "min", 0.1, 0.05)
    a = run_cascademscnn.parse_args(["--model", "kitti_car/cascade-mscnn-7s-576-2x", "--synthetic", "1", "--nms-type", "max", "--ovr-dnm", "min",
                                     "--nms-thr", "-0.5", "--det-thr", "0.2"])
    assert (a.nms_type, a.ovr_dnm, a.nms_thr, a.det_thr) == ("max", "min", -0.5, 0.2)
    a = run_cascademscnn.parse_args(["--model", "kitti_car/cascade-mscnn-7s-576-2x", "--synthetic", "1"])
    assert (a.nms_type, a.ovr_dnm, a.nms_thr) == ("maxg", "union", None)
    for mod in (run_mscnn_detection, run_cascademscnn):
        for bad in (["--nms-type", "ms"], ["--nms-type", "cover"], ["--ovr-dnm", "inter"]):
            with pytest.raises(SystemExit):
                mod.parse_args(["--model", "x", "--synthetic", "1"] + bad)


# ---- the witness ---------------------------------------------------------------------------------------------------------------------
def test_witness_reproduces_the_example_of_bbnms_for_type_max():
    """bbs = [0 0 1 1 1; .1 .1 1 1 1.1; 2 2 1 1 1], type 'max' (overlap .5, union): the second box outscores the first and overlaps it
    by .81 / 1.19, the third touches neither -> rows 2 and 3 remain, highest score first."""
    bbs = np.array([[0, 0, 1, 1, 1], [.1, .1, 1, 1, 1.1], [2, 2, 1, 1, 1]], np.float64)
    rows, order = wit.sort_rows(bbs)
    assert order.tolist() == [1, 0, 2]
    keep = wit.nms_max(rows, 0.5, greedy=False, ovr_dnm="union")
    assert keep.tolist() == [True, False, True]
    assert np.array_equal(rows[keep], bbs[[1, 2]])
    assert math.isclose(wit.overlaps(rows)[0, 1], 0.81 / 1.19, rel_tol=1e-12)
    assert math.isclose(wit.overlaps(rows, "min")[0, 1], 0.81, rel_tol=1e-12)


def test_witness_separates_greedy_from_non_greedy_and_union_from_min():
    chain = np.array([[0, 0, 10, 10, .9], [4, 0, 10, 10, .8], [8, 0, 10, 10, .7]], np.float64)      # A-B and B-C overlap 6/14, A-C 2/18
    assert wit.nms_max(chain, 0.4, True).tolist() == [True, False, True]
    assert wit.nms_max(chain, 0.4, False).tolist() == [True, False, False]
    nested = np.array([[0, 0, 20, 20, .9], [5, 5, 6, 6, .8]], np.float64)                          # 36 / 400 of the union, 36 / 36 of the smaller
    assert wit.nms_max(nested, 0.5, True, "union").tolist() == [True, True]
    assert wit.nms_max(nested, 0.5, True, "min").tolist() == [True, False]
    dead = np.array([[0, 0, 10, 10, .9], [2, 2, 0, 5, .8], [3, 3, -4, 5, .7], [1, 1, 10, 10, .6]], np.float64)
    assert wit.nms_max(dead, 0.5, False, "min").tolist() == [True, True, True, False]


def test_witness_agrees_with_the_oracle_greedy_union_stage_on_a_golden(orc):
    """The rows of the reference-made BoxOutput golden (boxout_dense_props) through the oracle's final stage: with nms_overlap = inf it
    returns every surviving row, sorted; the witness on those rows (greedy, union, 0.5 and 0.3) must pick what the oracle's own
    stage picks."""
    G = np.load(os.path.join(ROOT, "tests", "golden", "reference_layers.npz"))
    props = np.ascontiguousarray(G["boxout_dense_props"], np.float32)
    rng = np.random.default_rng(5)
    R = len(props)
    bbox_pred = (rng.standard_normal((R, 8)) * 0.5).astype(np.float32)
    cls_pred = (rng.standard_normal((R, 2)) * 2).astype(np.float32)
    kw = dict(cls_id=2, ratios=(576 / 375.0, 1920 / 1242.0), org_hw=(375, 1242))
    rows, ids = orc.detections(bbox_pred, cls_pred, props, nms_overlap=INF, **kw)
    assert len(rows) > 300 and np.all(np.diff(rows[:, 4]) <= 0)
    for ov in (0.5, 0.3):
        dets, kept = orc.detections(bbox_pred, cls_pred, props, nms_overlap=ov, **kw)
        keep = wit.nms_max(rows, ov, greedy=True, ovr_dnm="union")
        assert 0 < keep.sum() < len(rows)
        assert np.array_equal(ids[keep], kept) and np.array_equal(rows[keep].view(np.uint64), dets.view(np.uint64))
