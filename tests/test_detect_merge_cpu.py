"""Several forwards of an image, one NMS (mscnn_detections_candidates_*, mscnn_detections_merge_fwd, Net.detect_merge_*) without a
GPU: the struct mirrors, every refusal through the library with pointers nobody may touch and a NULL stream (each is decided before
any launch and names the offending value), the _bytes functions, the Net-level state errors on a graph-only net, the driver flags,
and the numpy witness (tests/merge_witness.py) against hand-computed cases."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import merge_witness as mw
from mscnn_amd import hipapi, net as mnet, zoo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
NAN = float("nan")
FAKE = C.c_void_p(0x1000)          # 16-byte aligned, never dereferenced: every call below is refused first
BIG = C.c_size_t(1 << 40)


def L():
    return hipapi.lib()


def err():
    return L().mscnn_last_error().decode()


def descs(S, ncls=2, cls_id=2, ratios=(1.0, 1.0), overlap=0.5):
    d = (hipapi.DetectionsDesc * max(S, 1))()
    for x in d:
        x.ncls, x.cls_id = ncls, cls_id
        x.ratio_h, x.ratio_w = ratios
        x.org_h, x.org_w = 375.0, 1242.0
        x.nms_overlap = overlap
        for k in range(4):
            x.bbox_std[k] = 0.1
    return d


def outs1(ncls=2):
    o = (hipapi.CascadeOutput * 1)()
    o[0].boxes = o[0].cls_prob = o[0].props = 0x1000
    o[0].ncls = ncls
    return o


def views(n, off_x=0.0, off_y=0.0, flip_x=0):
    v = (hipapi.DetectionsView * n)()
    for x in v:
        x.off_x, x.off_y, x.flip_x = off_x, off_y, flip_x
    return v


def add(desc=None, view=None, nms=None, pas=0, images=2, classes=2, blobs=FAKE, R=100, cand=FAKE, cap=300):
    desc = descs(images * classes) if desc is None else desc
    return L().mscnn_detections_candidates_add(desc, view, None if nms is None else C.byref(nms), pas, images, classes, blobs, blobs, blobs, R,
                                               cand, cap, None)


def cascade_add(desc=None, view=None, det_thr=0.0, nms=None, pas=0, images=2, outputs=1, classes=2, outs="default", R=100, cand=FAKE, cap=300):
    desc = descs(images * outputs * classes) if desc is None else desc
    outs = outs1() if outs == "default" else outs
    return L().mscnn_detections_candidates_cascade_add(desc, view, C.c_float(det_thr), None if nms is None else C.byref(nms), pas, images,
                                                       outputs, classes, outs, R, cand, cap, None)


def merge(overlap=None, nms=None, S=4, cand=FAKE, cap=300, pack=FAKE, ws=FAKE, ws_bytes=BIG):
    ov = (C.c_double * max(S, 1))(*([0.5] * max(S, 1))) if overlap is None else overlap
    return L().mscnn_detections_merge_fwd(ov, None if nms is None else C.byref(nms), S, cand, cap, pack, ws, ws_bytes, None)


# ---- the mirrors -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("header", ["include/mscnn_hip.h", "include/mscnn_net.h"])
def test_view_struct_mirrors_match_the_headers(header):
    text = open(os.path.join(ROOT, header)).read()
    m = re.search(r"typedef struct \{([^}]*)\}\s*mscnn_detections_view;", text)
    assert m and [d.strip() for d in m.group(1).split(";") if d.strip()] == ["double off_x, off_y", "int flip_x"]
    for S in (hipapi.DetectionsView, mnet.DetectionsView):
        assert [(n, t) for n, t in S._fields_] == [("off_x", C.c_double), ("off_y", C.c_double), ("flip_x", C.c_int)]
        assert C.sizeof(S) == 24 and [getattr(S, n).offset for n, _ in S._fields_] == [0, 8, 16]


def test_new_entry_points_are_exported():
    for name in ("mscnn_detections_candidates_bytes", "mscnn_detections_candidates_reset", "mscnn_detections_candidates_add",
                 "mscnn_detections_candidates_cascade_add", "mscnn_detections_merge_workspace_bytes", "mscnn_detections_merge_fwd"):
        assert hasattr(L(), name), name
    for name in ("mscnn_net_detect_merge_begin", "mscnn_net_detect_merge_add", "mscnn_net_detect_cascade_merge_add", "mscnn_net_detect_merge_end"):
        assert hasattr(mnet.lib(), name), name


def test_docs_say_that_there_is_no_pin_on_the_reference():
    for doc in ("include/mscnn_hip.h", "include/mscnn_net.h", "DESIGN.md", "INTEGRATION.md"):
        text = " ".join(open(os.path.join(ROOT, doc)).read().split())
        assert re.search(r"detect_merge|detections_merge", text), doc
        assert "no pin on the reference" in text.lower(), doc


# ---- the _bytes functions ----------------------------------------------------------------------------------------------------------------
def test_bytes_functions_grow_monotonically_and_return_0_for_refused_arguments():
    cb, wb = L().mscnn_detections_candidates_bytes, L().mscnn_detections_merge_workspace_bytes
    for f in (cb, wb):
        assert f(0, 100) == 0 and f(-1, 100) == 0 and f(1, 0) == 0 and f(4, -5) == 0
        assert f(1 << 16, 1 << 16) == 0                      # S * cand_cap past 2^31 - 1: the pack's row count is an int
        assert f(1, 1) > 0
    caps = [1, 63, 64, 65, 256, 1000, 4032, 4033, 6000, 20000]
    for S in (1, 4, 33):
        sizes = [cb(S, c) for c in caps]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
        assert all(cb(S, c) <= cb(S + 1, c) for c in caps)
        # a list holds a box (4 doubles), a float and an int per slot, and two ints per segment
        assert all(cb(S, c) >= S * (c * 40 + 8) for c in caps)
        for lo, hi in ((1, 4032), (4033, 20000)):            # within one path the workspace grows with the list ...
            w = [wb(S, c) for c in caps if lo <= c <= hi]
            assert all(a <= b for a, b in zip(w, w[1:])), (S, w)
    # ... and with the segments on the one-pass path; the tiled path holds one list at a time, whatever S is
    assert wb(1, 4032) < wb(4, 4032) < wb(33, 4032)
    assert wb(1, 4033) == wb(33, 4033) > 0
    assert wb(4, 4032) >= 4 * 4032 * (63 * 8 + 44)           # per segment: the bit matrix and the sorted list


# ---- refusals: the add calls -------------------------------------------------------------------------------------------------------------
def test_add_refuses_null_pointers_and_bad_counts():
    assert add(cand=None) != 0 and "null pointer" in err()
    assert add(blobs=None) != 0 and "null pointer" in err()
    assert L().mscnn_detections_candidates_add(None, None, None, 0, 2, 2, FAKE, FAKE, FAKE, 100, FAKE, 300, None) != 0 and "null pointer" in err()
    assert add(images=0) != 0 and "0 images x 2 classes" in err()
    assert add(classes=-3) != 0 and "2 images x -3 classes" in err()
    assert add(cap=0) != 0 and "cand_cap 0" in err()
    assert add(cap=-7) != 0 and "cand_cap -7" in err()
    assert add(R=0) != 0 and "R_all = 0" in err()
    assert cascade_add(cand=None) != 0 and "null pointer" in err()
    assert cascade_add(outs=None) != 0 and "null pointer" in err()
    assert cascade_add(outputs=0) != 0 and "0 cascade outputs" in err()
    assert cascade_add(outputs=5, desc=descs(20)) != 0 and "5 cascade outputs" in err()
    assert cascade_add(cap=0) != 0 and "cand_cap 0" in err()
    o = outs1()
    o[0].props = None
    assert cascade_add(outs=o) != 0 and "output 0 of 1: null pointer" in err()


@pytest.mark.parametrize("call", [add, cascade_add])
def test_add_refuses_a_pass_or_a_row_count_the_tag_can_not_hold(call):
    assert call(pas=-1) != 0 and "pass -1" in err()
    assert call(pas=128) != 0 and "pass 128" in err()
    assert call(R=1 << 24, cap=1 << 25) != 0 and f"R_all = {1 << 24}" in err() and "24 row bits" in err()


@pytest.mark.parametrize("call", [add, cascade_add])
@pytest.mark.parametrize("ratios,text", [((NAN, 1.0), "nan x 1"), ((1.0, 0.0), "1 x 0"), ((-2.0, 1.0), "-2 x 1"), ((1.0, NAN), "1 x nan")])
def test_add_refuses_a_nan_or_non_positive_ratio(call, ratios, text):
    d = descs(4)
    d[2].ratio_h, d[2].ratio_w = ratios
    assert call(desc=d) != 0
    assert "segment 2: ratios " + text in err(), err()


@pytest.mark.parametrize("call", [add, cascade_add])
def test_add_refuses_a_non_finite_offset_and_a_flip_that_is_no_flag(call):
    for ox, oy, text in ((INF, 0.0, "(inf, 0)"), (0.0, NAN, "(0, nan)"), (-INF, 3.0, "(-inf, 3)")):
        v = views(2)
        v[1].off_x, v[1].off_y = ox, oy
        assert call(view=v) != 0 and "image 1: view offset " + text in err(), err()
    for f in (2, -1):
        v = views(2)
        v[0].flip_x = f
        assert call(view=v) != 0 and f"image 0: flip_x {f}" in err(), err()


@pytest.mark.parametrize("call", [add, cascade_add])
def test_add_refuses_an_unaligned_candidate_buffer_and_a_bad_class(call):
    assert call(cand=C.c_void_p(0x1008)) != 0 and "cand must be 16-byte aligned" in err()
    d = descs(4)
    d[3].cls_id = 3
    assert call(desc=d) != 0 and "cls_id 3 of 2" in err()


def test_add_passes_the_nms_params_refusals_on_and_the_cascade_add_refuses_the_plain_det_thr():
    for p, match in ((hipapi.NmsParams(2, 0, -INF, 0.0), r"type 2 \('ms'\)"), (hipapi.NmsParams(0, 2, -INF, 0.0), "ovr_dnm 2 "),
                     (hipapi.NmsParams(0, 0, NAN, 0.0), "thr is NaN")):
        for call in (add, cascade_add, merge):
            assert call(nms=p) != 0 and re.search(match, err()), err()
    p = hipapi.NmsParams(0, 0, -INF, 0.5)
    assert cascade_add(nms=p) != 0 and "det_thr 0.5 is the plain stage's" in err()
    assert L().mscnn_detections_candidates_reset(None, 4, 10, None) != 0 and "null pointer" in err()
    assert L().mscnn_detections_candidates_reset(FAKE, 0, 10, None) != 0 and "0 segments" in err()
    assert L().mscnn_detections_candidates_reset(FAKE, 4, 0, None) != 0 and "cand_cap 0" in err()
    assert L().mscnn_detections_candidates_reset(C.c_void_p(0x1004), 4, 10, None) != 0 and "16-byte aligned" in err()


# ---- refusals: the merge -----------------------------------------------------------------------------------------------------------------
def test_merge_refusals_name_the_value():
    assert merge(cand=None) != 0 and "null pointer" in err()
    assert merge(pack=None) != 0 and "null pointer" in err()
    assert merge(ws=None) != 0 and "null pointer" in err()
    assert L().mscnn_detections_merge_fwd(None, None, 4, FAKE, 300, FAKE, FAKE, BIG, None) != 0 and "null pointer" in err()
    assert merge(S=0) != 0 and "0 segments" in err()
    assert merge(S=-2) != 0 and "-2 segments" in err()
    assert merge(cap=0) != 0 and "cand_cap 0" in err()
    ov = (C.c_double * 4)(0.5, 0.5, NAN, 0.5)
    assert merge(overlap=ov) != 0 and "segment 2: nms_overlap is NaN" in err()
    for which in ("cand", "ws", "pack"):
        assert merge(**{which: C.c_void_p(0x1008)}) != 0 and "must be 16-byte aligned" in err(), which
    need = L().mscnn_detections_merge_workspace_bytes(4, 300)
    assert merge(ws_bytes=C.c_size_t(need - 1)) != 0 and f"workspace {need - 1} < {need}" in err()
    need = L().mscnn_detections_merge_workspace_bytes(4, 5000)
    assert merge(cap=5000, ws_bytes=C.c_size_t(need - 1)) != 0 and f"workspace {need - 1} < {need}" in err()


def test_merge_above_4032_slots_refuses_a_non_default_type_or_denominator_naming_the_limit():
    for p, text in ((hipapi.NmsParams(1, 0, -INF, 0.0), "type 1, ovr_dnm 0"), (hipapi.NmsParams(0, 1, -INF, 0.0), "type 0, ovr_dnm 1")):
        assert merge(nms=p, cap=4033) != 0
        assert "4033 slots > 4032" in err() and text in err(), err()
    # (4032 slots take the one-pass path, which has every mode: nothing to refuse but the too small workspace handed in here)
    assert merge(nms=hipapi.NmsParams(1, 1, -INF, 0.0), cap=4032, ws_bytes=C.c_size_t(16)) != 0 and "workspace 16 <" in err()


# ---- the Net-level state errors on a graph-only net --------------------------------------------------------------------------------------
def test_net_state_errors_are_decided_before_the_device_is_touched():
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=96, width=320), device=-1)
    kw = [dict(ratios=(1.0, 1.0), org_hw=(96, 320))]
    with pytest.raises(mnet.NetError, match="detect_merge_add: no merge is open"):
        n.detect_merge_add(kw, [2])
    with pytest.raises(mnet.NetError, match="detect_cascade_merge_add: no merge is open"):
        n.detect_cascade_merge_add(kw, [("a", "b", "c")], [2])
    with pytest.raises(mnet.NetError, match="detect_merge_end: no merge is open"):
        n.detect_merge_end()
    with pytest.raises(mnet.NetError, match="0 images x 1 classes"):
        n.detect_merge_begin(0, 1, 100)
    with pytest.raises(mnet.NetError, match="cand_cap 0"):
        n.detect_merge_begin(1, 1, 0)
    with pytest.raises(mnet.NetError, match=r"device -1 \(graph only\)"):
        n.detect_merge_begin(1, 1, 100)
    with pytest.raises(mnet.NetError, match="detect_merge_end: no merge is open"):      # (the refused begin opened nothing)
        n.detect_merge_end()
    with pytest.raises(mnet.NetError, match="2 views for 1 images"):
        n.detect_merge_add(kw, [2], views=[{}, {}])


def test_driver_flags_parse():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import run_cascademscnn
        import run_mscnn_detection
    finally:
        sys.path.pop(0)
    for mod, model in ((run_mscnn_detection, "caltech/mscnn-7s-480"), (run_cascademscnn, "kitti_car/cascade-mscnn-7s-576-2x")):
        a = mod.parse_args(["--model", model, "--synthetic", "1"])
        assert a.scales is None and a.flip is False
        a = mod.parse_args(["--model", model, "--synthetic", "1", "--scales", "384x1280,576x1920", "--flip"])
        assert a.scales == [(384, 1280), (576, 1920)] and a.flip is True
        for bad in ("384", "384x", "0x64", "axb", "384x1280,"):
            with pytest.raises(SystemExit):
                mod.parse_args(["--model", model, "--synthetic", "1", "--scales", bad])


# ---- the witness against hand-computed cases --------------------------------------------------------------------------------------------
def plain_blobs(xywh, logit):
    """ROI blobs (ncls = 2) whose transformed boxes are the given integer [x y w h] (zero regression, ratio 1) with class-2
    probability sigmoid(logit)."""
    xywh = np.asarray(xywh, np.float32).reshape(-1, 4)
    R = len(xywh)
    props = np.zeros((R, 6), np.float32)
    props[:, 1:3] = xywh[:, :2]
    props[:, 3:5] = xywh[:, :2] + xywh[:, 2:]
    cls_pred = np.zeros((R, 2), np.float32)
    cls_pred[:, 1] = logit
    return np.zeros((R, 8), np.float32), cls_pred, props


def test_witness_rows_come_back_in_row_order_with_the_thresholds_applied():
    blobs = plain_blobs([[10, 10, 20, 20], [100, 10, 20, 20], [200, 10, 20, 20]], [0.0, 2.0, 1.0])
    rows, ids = mw.plain_rows(*blobs, 2, org_hw=(1000, 1000))
    assert ids.tolist() == [0, 1, 2] and np.array_equal(rows[:, :4], [[10, 10, 20, 20], [100, 10, 20, 20], [200, 10, 20, 20]])
    assert rows[0, 4] == 0.5 and rows[1, 4] > rows[2, 4] > 0.5
    rows, ids = mw.plain_rows(*blobs, 2, org_hw=(1000, 1000), thr=0.5)              # strict
    assert ids.tolist() == [1, 2]
    rows, ids = mw.plain_rows(*blobs, 2, org_hw=(1000, 1000), det_thr=0.5)          # >=
    assert ids.tolist() == [0, 1, 2]
    rows, ids = mw.plain_rows(*[b[:0] for b in blobs], 2)
    assert rows.shape == (0, 5) and len(ids) == 0


def test_witness_cascade_rows_by_hand():
    boxes = np.array([[0, 10, 20, 29, 59], [0, -5, 20, 2000, 59], [0, 10, 20, 29, 59]], np.float32)
    props = boxes.copy()
    props[2, 3] = props[2, 1] - 1                                                  # zero width: dropped (:114)
    prob = np.array([[.25, .75], [.5, .5], [.1, .9]], np.float32)
    rows, ids = mw.cascade_rows(boxes, prob, props, 2, ratios=(2.0, 2.0), org_hw=(100, 200))
    assert ids.tolist() == [0, 1]
    assert rows.tolist() == [[5.0, 10.0, 10.5, 20.5, 0.75], [0.0, 10.0, 201.0, 20.5, 0.5]]      # x2 clipped to 200: w = 200 - 0 + 1
    rows, ids = mw.cascade_rows(boxes, prob, props, 2, ratios=(2.0, 2.0), org_hw=(100, 200), det_thr=0.75)
    assert ids.tolist() == [0]


def test_witness_two_identical_passes_give_the_single_pass_result_with_every_tag_from_pass_0():
    rng = np.random.default_rng(3)
    xy = rng.integers(0, 60, (40, 2))
    blobs = plain_blobs(np.concatenate([xy, rng.integers(10, 30, (40, 2))], 1), rng.permutation(np.linspace(-2, 2, 40)))
    rows, ids = mw.plain_rows(*blobs, 2, org_hw=(1000, 1000))
    for t in ("maxg", "max"):
        for dn in ("union", "min"):
            one = mw.merge([(rows, ids)], 0.5, t, dn)
            two = mw.merge([(rows, ids), (rows, ids)], 0.5, t, dn)
            assert 0 < len(one[0]) < len(rows)
            assert np.array_equal(one[0], two[0]) and np.array_equal(one[2], two[2])
            assert two[1].tolist() == [0] * len(one[0]) and (one[3], two[3]) == (40, 80)


def test_witness_a_mirrored_box_maps_back_onto_its_original():
    """A box [x y w h] in a frame of width W shows at [W - (x + w), y, w, h] in the mirrored frame; the flip view takes it back."""
    W = 640
    box = np.array([[100.0, 50.0, 30.0, 40.0, 0.9], [0.0, 0.0, 640.0, 10.0, 0.8]])
    mirrored = box.copy()
    mirrored[:, 0] = W - (box[:, 0] + box[:, 2])
    assert mirrored[:, 0].tolist() == [510.0, 0.0]
    back = mw.apply_view(mirrored, W, (0.0, 0.0, 1))
    assert np.array_equal(back, box)
    assert np.array_equal(mw.apply_view(box, W, None), box) and mw.apply_view(box, W, None) is not box
    # merged with the unmirrored pass: the copy of pass 1 is suppressed by the equal-scored original of pass 0 (the tie rule)
    dets, pas, row, cands = mw.merge([(box, [0, 1]), (back, [0, 1])])
    assert np.array_equal(dets, box) and pas.tolist() == [0, 0] and row.tolist() == [0, 1] and cands == 4
    dets, pas, row, _ = mw.merge([(back[::-1], [0, 1]), (box, [0, 1])])                       # the other order: again the first pass wins
    assert np.array_equal(dets, box) and pas.tolist() == [0, 0] and row.tolist() == [1, 0]


def test_witness_a_tile_offset_is_applied_after_the_flip_and_leaves_size_and_prob_alone():
    rows = np.array([[10.0, 20.0, 30.0, 40.0, 0.5]])
    assert mw.apply_view(rows, 100, (1000.0, 2000.0, 0)).tolist() == [[1010.0, 2020.0, 30.0, 40.0, 0.5]]
    assert mw.apply_view(rows, 100, (1000.0, 2000.0, 1)).tolist() == [[1060.0, 2020.0, 30.0, 40.0, 0.5]]      # 100 - 40 + 1000
    assert mw.apply_view(rows, 100, (0.25, -0.5, 0)).tolist() == [[10.25, 19.5, 30.0, 40.0, 0.5]]
    # two tiles that see the same object: in tile coordinates the boxes are far apart, in the frame they coincide
    a = mw.apply_view(np.array([[90.0, 10.0, 20.0, 20.0, 0.9]]), 128, (0.0, 0.0, 0))
    b = mw.apply_view(np.array([[26.0, 10.0, 20.0, 20.0, 0.7]]), 128, (64.0, 0.0, 0))
    dets, pas, row, _ = mw.merge([(a, [5]), (b, [9])])
    assert dets.tolist() == [[90.0, 10.0, 20.0, 20.0, 0.9]] and pas.tolist() == [0] and row.tolist() == [5]
    facts = mw.cross_pass_facts([(a, [5]), (b, [9])])
    assert facts == (True, False, {0})
