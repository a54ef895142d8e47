"""The views of a frame run as one batch (mscnn_preprocess_views_u8_f32, mscnn_detections_candidates_add_views /
_cascade_add_views, Net.set_image_views, Net.detect_merge_add(..., list_of=), tile_views) without a GPU: the exports and struct
mirrors, every refusal through the libraries with pointers nobody may touch and a NULL stream (each is decided before any launch and
names the offending value), the workspace size, the pure tile helper, the driver flags and the numpy witness's self-checks."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import views_witness as vw
from mscnn_amd import hipapi, net as mnet, zoo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(0x1000)          # 16-byte aligned, never dereferenced: every call below is refused first
BIG = C.c_size_t(1 << 40)
MEAN = (C.c_float * 3)(104.0, 117.0, 123.0)


def L():
    return hipapi.lib()


def err():
    return L().mscnn_last_error().decode()


# ---- exports, mirrors, docs -------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_exported_and_declared():
    hip_h = open(os.path.join(ROOT, "include/mscnn_hip.h")).read()
    net_h = open(os.path.join(ROOT, "include/mscnn_net.h")).read()
    for name in ("mscnn_preprocess_views_workspace_bytes", "mscnn_preprocess_views_u8_f32", "mscnn_detections_candidates_add_views",
                 "mscnn_detections_candidates_cascade_add_views"):
        assert hasattr(L(), name), name
        assert re.search(r"MSCNN_API\s+\w+\s+" + name + r"\(", hip_h), name
    for name in ("mscnn_net_set_image_views", "mscnn_net_detect_merge_add_views", "mscnn_net_detect_cascade_merge_add_views"):
        assert hasattr(mnet.lib(), name), name
        assert re.search(r"MSCNN_NET_API\s+\w+\s+" + name + r"\(", net_h), name


@pytest.mark.parametrize("header", ["include/mscnn_hip.h", "include/mscnn_net.h"])
def test_view_struct_mirrors_match_the_headers(header):
    text = open(os.path.join(ROOT, header)).read()
    m = re.search(r"typedef struct \{([^}]*)\}\s*mscnn_preprocess_view;", text)
    assert m and [d.strip() for d in m.group(1).split(";") if d.strip()] == ["int frame", "int x0, y0, w, h", "int flip_x"]
    for S in (hipapi.PreprocessView, mnet.PreprocessView):
        assert [n for n, _ in S._fields_] == ["frame", "x0", "y0", "w", "h", "flip_x"] and all(t is C.c_int for _, t in S._fields_)
        assert C.sizeof(S) == 24


def test_docs_name_the_views_calls_the_order_rule_and_that_there_is_no_pin_on_the_reference():
    for doc in ("include/mscnn_hip.h", "include/mscnn_net.h", "DESIGN.md", "INTEGRATION.md", "README.md"):
        text = " ".join(open(os.path.join(ROOT, doc)).read().split())
        assert re.search(r"add_views|set_image_views", text), doc
    for doc in ("include/mscnn_hip.h", "include/mscnn_net.h", "DESIGN.md", "INTEGRATION.md"):
        text = " ".join(open(os.path.join(ROOT, doc)).read().split())
        assert re.search(r"neither views nor a merge", text), doc
        assert re.search(r"\(add call, image index ascending, row\)", text), doc


# ---- mscnn_preprocess_views_*: refusals and the workspace ----------------------------------------------------------------------------------
def views(*specs):
    return hipapi.view_array([dict(zip(("frame", "x0", "y0", "w", "h", "flip_x"), s)) for s in specs])


def pre(v=None, count=None, frames="default", org=((37, 53), (41, 29)), num_frames=None, out=FAKE, H=24, W=40, mean=MEAN, ws=FAKE, wb=BIG,
        oh="default", ow="default"):
    v = views((0, 0, 0, 53, 37, 0), (1, 2, 3, 20, 30, 1)) if v is None else v
    count = len(v) if count is None else count
    F = len(org)
    fr = (C.c_void_p * F)(*([0x2000] * F)) if frames == "default" else frames
    oh = (C.c_int * F)(*[o[0] for o in org]) if oh == "default" else oh
    ow = (C.c_int * F)(*[o[1] for o in org]) if ow == "default" else ow
    return L().mscnn_preprocess_views_u8_f32(fr, oh, ow, F if num_frames is None else num_frames, v, count, out, H, W, mean, ws, wb, None)


def test_preprocess_views_refuses_null_pointers_and_bad_counts():
    for kw in (dict(frames=None), dict(oh=None), dict(ow=None), dict(out=None), dict(mean=None), dict(ws=None)):
        assert pre(**kw) != 0 and "null pointer" in err(), kw
    assert L().mscnn_preprocess_views_u8_f32((C.c_void_p * 1)(0x2000), (C.c_int * 1)(5), (C.c_int * 1)(5), 1, None, 1, FAKE, 4, 4, MEAN, FAKE, BIG,
                                             None) != 0 and "null pointer" in err()
    assert pre(count=0) != 0 and "count 0 < 1" in err()
    assert pre(count=-2) != 0 and "count -2 < 1" in err()
    assert pre(num_frames=0) != 0 and "num_frames 0 < 1" in err()
    assert pre(H=0) != 0 and "bad output shape 0 x 40" in err()
    assert pre(W=-1) != 0 and "bad output shape 24 x -1" in err()
    fr = (C.c_void_p * 2)(0x2000, None)
    assert pre(frames=fr) != 0 and "frame 1 is a null pointer" in err()
    assert pre(org=((37, 53), (0, 29))) != 0 and "frame 1 has bad shape 0 x 29" in err()


def test_preprocess_views_refuses_a_bad_view_naming_it():
    assert pre(views((0, 0, 0, 53, 37, 0), (2, 0, 0, 5, 5, 0))) != 0 and "view 1: frame 2 outside [0, 2)" in err()
    assert pre(views((-1, 0, 0, 5, 5, 0))) != 0 and "view 0: frame -1 outside [0, 2)" in err()
    assert pre(views((0, 0, 0, 0, 5, 0))) != 0 and "view 0: window 5 x 0 (h x w) is empty" in err()
    assert pre(views((0, 0, 0, 5, -3, 0))) != 0 and "view 0: window -3 x 5 (h x w) is empty" in err()
    for spec, frame in (((0, 50, 0, 4, 5, 0), "frame 0 of 37 x 53"), ((0, 0, 33, 4, 5, 0), "frame 0 of 37 x 53"), ((1, -1, 0, 4, 5, 0), "frame 1 of 41 x 29"),
                        ((1, 0, -2, 4, 5, 0), "frame 1 of 41 x 29"), ((1, 0, 0, 30, 41, 0), "frame 1 of 41 x 29"),
                        ((0, 2 ** 31 - 2, 0, 4, 5, 0), "frame 0 of 37 x 53")):
        assert pre(views((0, 0, 0, 53, 37, 0), spec)) != 0
        assert f"view 1: window {spec[4]} x {spec[3]} (h x w) at (x0 {spec[1]}, y0 {spec[2]}) is not inside {frame}" in err(), err()
    # (a window touching the last row and column passes the view checks: the next refusal is the workspace's)
    assert pre(views((0, 49, 32, 4, 5, 0)), wb=C.c_size_t(0)) != 0 and "workspace 0 bytes <" in err()
    for f in (2, -1):
        assert pre(views((0, 0, 0, 5, 5, f))) != 0 and f"view 0: flip_x {f} (0 or 1)" in err()


def test_preprocess_views_workspace_is_sized_per_view_and_refused_when_small_or_unaligned():
    wbf = L().mscnn_preprocess_views_workspace_bytes
    one = L().mscnn_preprocess_workspace_bytes
    one.restype = C.c_size_t
    al = lambda b: (b + 255) // 256 * 256      # noqa: E731
    v = views((0, 0, 0, 53, 37, 0), (1, 2, 3, 20, 30, 1), (0, 5, 3, 31, 20, 0), (0, 7, 0, 1, 37, 0))
    sizes = [wbf(v, k, 24, 40) for k in range(1, 5)]
    assert sizes == [sum(al(one(v[i].h, v[i].w, 24, 40)) for i in range(k)) for k in range(1, 5)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and all(s % 256 == 0 for s in sizes)
    # 0 for arguments the op refuses
    assert wbf(None, 1, 24, 40) == 0 and wbf(v, 0, 24, 40) == 0 and wbf(v, -1, 24, 40) == 0 and wbf(v, 4, 0, 40) == 0 and wbf(v, 4, 24, -5) == 0
    assert wbf(views((0, 0, 0, 0, 5, 0)), 1, 24, 40) == 0 and wbf(views((0, 0, 0, 5, 5, 0), (0, 0, 0, 5, 0, 0)), 2, 24, 40) == 0
    need = sizes[1]
    assert pre(wb=C.c_size_t(need - 1)) != 0 and f"workspace {need - 1} bytes < {need}" in err()
    assert pre(ws=C.c_void_p(0x1008)) != 0 and "workspace must be 16-byte aligned" in err()


# ---- mscnn_detections_candidates_add_views / _cascade_add_views: refusals ------------------------------------------------------------------
def descs(S, ncls=2, cls_id=2, ratios=(1.0, 1.0)):
    d = (hipapi.DetectionsDesc * max(S, 1))()
    for x in d:
        x.ncls, x.cls_id = ncls, cls_id
        x.ratio_h, x.ratio_w = ratios
        x.org_h, x.org_w = 375.0, 1242.0
        x.nms_overlap = 0.5
        for k in range(4):
            x.bbox_std[k] = 0.1
    return d


def outs1(ncls=2):
    o = (hipapi.CascadeOutput * 1)()
    o[0].boxes = o[0].cls_prob = o[0].props = 0x1000
    o[0].ncls = ncls
    return o


def lof(*v):
    return (C.c_int * len(v))(*v)


def add(desc=None, view=None, list_of="default", nms=None, pas=0, images=3, lists=2, classes=2, blobs=FAKE, R=100, cand=FAKE, cap=300):
    desc = descs(images * classes) if desc is None else desc
    list_of = lof(0, 1, 0) if list_of == "default" else list_of
    return L().mscnn_detections_candidates_add_views(desc, view, list_of, None if nms is None else C.byref(nms), pas, images, lists, classes, blobs,
                                                     blobs, blobs, R, cand, cap, None)


def cascade_add(desc=None, view=None, list_of="default", det_thr=0.0, nms=None, pas=0, images=3, lists=2, outputs=1, classes=2, outs="default",
                R=100, cand=FAKE, cap=300):
    desc = descs(images * outputs * classes) if desc is None else desc
    list_of = lof(0, 1, 0) if list_of == "default" else list_of
    outs = outs1() if outs == "default" else outs
    return L().mscnn_detections_candidates_cascade_add_views(desc, view, list_of, C.c_float(det_thr), None if nms is None else C.byref(nms), pas,
                                                             images, lists, outputs, classes, outs, R, cand, cap, None)


@pytest.mark.parametrize("call", [add, cascade_add])
def test_add_views_refuses_what_is_new(call):
    assert call(list_of=None) != 0 and "null pointer (list_of)" in err()
    assert call(lists=0) != 0 and "num_lists 0 < 1" in err()
    assert call(lists=-4) != 0 and "num_lists -4 < 1" in err()
    assert call(list_of=lof(0, 2, 0)) != 0 and "image 1: list_of 2 outside [0, 2)" in err()
    assert call(list_of=lof(0, 1, -1)) != 0 and "image 2: list_of -1 outside [0, 2)" in err()
    assert call(lists=1 << 24) != 0 and f"{1 << 24} lists x 2 slots" in err()
    assert call(lists=1 << 20, cap=1 << 12) != 0 and "is past 2^31 - 1" in err()


@pytest.mark.parametrize("call", [add, cascade_add])
def test_add_views_refuses_everything_the_add_calls_refuse(call):
    assert call(cand=None) != 0 and "null pointer" in err()
    assert call(images=0, list_of=lof(0)) != 0 and "0 images x 2 classes" in err()
    assert call(classes=-3) != 0 and "3 images x -3 classes" in err()
    assert call(cap=0) != 0 and "cand_cap 0" in err()
    assert call(R=0) != 0 and "R_all = 0" in err()
    assert call(R=1 << 24, cap=1 << 25) != 0 and "24 row bits" in err()
    assert call(pas=-1) != 0 and "pass -1" in err()
    assert call(pas=128) != 0 and "pass 128" in err()
    assert call(cand=C.c_void_p(0x1008)) != 0 and "cand must be 16-byte aligned" in err()
    d = descs(6)
    d[5].ratio_h = float("nan")
    assert call(desc=d) != 0 and "segment 5: ratios nan x 1" in err()      # (the descs are this forward's: 3 images x 2 slots)
    d = descs(6)
    d[4].cls_id = 3
    assert call(desc=d) != 0 and "cls_id 3 of 2" in err()
    v = (hipapi.DetectionsView * 3)()
    v[2].off_x = float("inf")
    assert call(view=v) != 0 and "image 2: view offset (inf, 0)" in err()
    v = (hipapi.DetectionsView * 3)()
    v[1].flip_x = 2
    assert call(view=v) != 0 and "image 1: flip_x 2" in err()
    assert call(nms=hipapi.NmsParams(2, 0, -float("inf"), 0.0)) != 0 and "type 2 ('ms')" in err()


def test_add_views_the_two_forms_refuse_their_own():
    assert add(blobs=None) != 0 and "null pointer" in err()
    assert cascade_add(outs=None) != 0 and "null pointer" in err()
    assert cascade_add(outputs=5, desc=descs(30)) != 0 and "5 cascade outputs" in err()
    assert cascade_add(nms=hipapi.NmsParams(0, 0, -float("inf"), 0.5)) != 0 and "det_thr 0.5 is the plain stage's" in err()
    for call, name in ((add, "detections_candidates_add_views:"), (cascade_add, "detections_candidates_cascade_add_views:")):
        assert call(cap=-7) != 0 and err().startswith(name), err()


# ---- Net level on a graph-only net ---------------------------------------------------------------------------------------------------------
def test_net_set_image_views_refuses_before_touching_the_device():
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=96, width=320), device=-1)
    f = np.zeros((37, 53, 3), np.uint8)
    whole = dict(x0=0, y0=0, w=53, h=37)
    with pytest.raises(mnet.NetError, match="2 views for blob data of shape 1 3 96 320"):
        n.set_image_views("data", [f], [whole, whole])
    with pytest.raises(mnet.NetError, match="0 views for blob data"):
        n.set_image_views("data", [f], [])
    with pytest.raises(mnet.NetError, match="Unknown blob name nope"):
        n.set_image_views("nope", [f], [whole])
    with pytest.raises(mnet.NetError, match="num_frames 0"):
        n.set_image_views("data", [], [whole])
    with pytest.raises(mnet.NetError, match=r"view 0: frame 1 outside \[0, 1\)"):
        n.set_image_views("data", [f], [dict(whole, frame=1)])
    with pytest.raises(mnet.NetError, match=r"view 0: window 37 x 54 \(h x w\) at \(x0 0, y0 0\) is empty or not inside frame 0 of 37 x 53"):
        n.set_image_views("data", [f], [dict(whole, w=54)])
    with pytest.raises(mnet.NetError, match=r"view 0: window 0 x 53 \(h x w\)"):
        n.set_image_views("data", [f], [dict(whole, h=0)])
    with pytest.raises(mnet.NetError, match=r"at \(x0 -1, y0 0\)"):
        n.set_image_views("data", [f], [dict(whole, x0=-1, w=5)])
    with pytest.raises(mnet.NetError, match=r"view 0: flip_x 3 \(0 or 1\)"):
        n.set_image_views("data", [f], [dict(whole, flip_x=3)])
    with pytest.raises(mnet.NetError, match="frame 0 is not a uint8"):
        n.set_image_views("data", [f.astype(np.float32)], [whole])
    with pytest.raises(mnet.NetError, match=r"device -1 \(graph only\)"):      # (everything else is fine: the device would be next)
        n.set_image_views("data", [f], [whole])
    n.reshape_input("data", (2, 3, 96, 320))
    with pytest.raises(mnet.NetError, match="1 views for blob data of shape 2 3 96 320"):
        n.set_image_views("data", [f], [whole])


def test_net_add_views_state_errors_are_decided_before_the_device_is_touched():
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=96, width=320), device=-1)
    kw = [dict(ratios=(1.0, 1.0), org_hw=(96, 320))]
    with pytest.raises(mnet.NetError, match="detect_merge_add_views: no merge is open"):
        n.detect_merge_add(kw, [2], list_of=[0])
    with pytest.raises(mnet.NetError, match="detect_cascade_merge_add_views: no merge is open"):
        n.detect_cascade_merge_add(kw, [("a", "b", "c")], [2], list_of=[0])
    with pytest.raises(mnet.NetError, match="2 list_of entries for 1 images"):
        n.detect_merge_add(kw, [2], list_of=[0, 0])
    with pytest.raises(mnet.NetError, match="detect_merge_add: no merge is open"):      # (without the keyword: the call it always was)
        n.detect_merge_add(kw, [2])


# ---- tile_views ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(120, 400), (375, 1242), (1080, 1920), (37, 53)])
@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 2), (2, 2), (3, 4)])
@pytest.mark.parametrize("overlap", [0, 1, 7])
@pytest.mark.parametrize("flip", [False, True])
def test_tile_views_are_equal_sized_inside_the_frame_and_cover_it(hw, rows, cols, overlap, flip):
    views, params, mviews = mnet.tile_views(hw, rows, cols, overlap=overlap, flip=flip, input_hw=(96, 320))
    N = rows * cols * (2 if flip else 1)
    assert len(views) == len(params) == len(mviews) == N
    sizes = {(v["h"], v["w"]) for v in views}
    assert len(sizes) == 1
    (th, tw), = sizes
    cover = np.zeros(hw, np.int32)
    for v, p, m in zip(views, params, mviews):
        assert 0 <= v["x0"] and 0 <= v["y0"] and v["x0"] + v["w"] <= hw[1] and v["y0"] + v["h"] <= hw[0] and v["frame"] == 0
        assert p["org_hw"] == (th, tw) and p["ratios"] == (96 / th, 320 / tw)
        assert (m["off_x"], m["off_y"], m["flip_x"]) == (float(v["x0"]), float(v["y0"]), v["flip_x"])
        if not v["flip_x"]:
            cover[v["y0"]:v["y0"] + th, v["x0"]:v["x0"] + tw] += 1
    assert cover.min() >= 1, "a pixel of the frame is in no tile"
    assert [v["flip_x"] for v in views] == [0] * (rows * cols) + [1] * (N - rows * cols)
    if flip:      # the mirrors follow the tiles in the tiles' order
        assert [(v["x0"], v["y0"]) for v in views[:rows * cols]] == [(v["x0"], v["y0"]) for v in views[rows * cols:]]
    # neighbours share at least `overlap` columns / rows (the last one, shifted inwards, may share more), and nothing is wasted:
    # one pixel less per tile would not cover the frame with this overlap
    xs = sorted({v["x0"] for v in views}); ys = sorted({v["y0"] for v in views})
    assert len(xs) == cols and len(ys) == rows and xs[-1] == hw[1] - tw and ys[-1] == hw[0] - th
    assert all(a + tw - b >= overlap for a, b in zip(xs, xs[1:])) and all(a + th - b >= overlap for a, b in zip(ys, ys[1:]))
    assert cols * (tw - 1) - (cols - 1) * overlap < hw[1] and rows * (th - 1) - (rows - 1) * overlap < hw[0]


def test_tile_views_the_issue_case_and_the_refusals():
    views, params, mviews = mnet.tile_views((120, 400), 1, 2, overlap=40, flip=True)
    assert [(v["x0"], v["y0"], v["w"], v["h"], v["flip_x"]) for v in views] == [(0, 0, 220, 120, 0), (180, 0, 220, 120, 0), (0, 0, 220, 120, 1),
                                                                              (180, 0, 220, 120, 1)]
    assert params == [dict(org_hw=(120, 220))] * 4 and [m["off_x"] for m in mviews] == [0.0, 180.0, 0.0, 180.0]
    assert mnet.tile_views((100, 101), 1, 3)[0][2]["x0"] == 101 - 34      # the last column is shifted inwards, not shrunk
    for bad in (dict(rows=0, cols=1), dict(rows=1, cols=-1), dict(rows=1, cols=2, overlap=-1), dict(rows=1, cols=2, overlap=400),
                dict(rows=121, cols=1), dict(rows=1, cols=401)):
        with pytest.raises(ValueError):
            mnet.tile_views((120, 400), **bad)


# ---- the drivers' flags ------------------------------------------------------------------------------------------------------------------------
def test_driver_flags_parse():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import run_cascademscnn
        import run_mscnn_detection
    finally:
        sys.path.pop(0)
    for mod, model in ((run_mscnn_detection, "caltech/mscnn-7s-480"), (run_cascademscnn, "kitti_car/cascade-mscnn-7s-576-2x")):
        a = mod.parse_args(["--model", model, "--synthetic", "1"])
        assert a.tiles is None and a.views_batch is False
        a = mod.parse_args(["--model", model, "--synthetic", "1", "--tiles", "2x3:16", "--views-batch", "--flip"])
        assert a.tiles == (2, 3, 16) and a.views_batch is True and a.flip is True
        assert mod.parse_args(["--model", model, "--synthetic", "1", "--tiles", "1x2"]).tiles == (1, 2, 0)
        for bad in ("2", "2x", "0x2", "axb", "2x2:", "2x2:-1", "2x2:a"):
            with pytest.raises(SystemExit):
                mod.parse_args(["--model", model, "--synthetic", "1", "--tiles", bad])
        with pytest.raises(SystemExit):      # nothing to batch
            mod.parse_args(["--model", model, "--synthetic", "1", "--views-batch"])


# ---- the witness ------------------------------------------------------------------------------------------------------------------------------
def test_witness_self_checks():
    vw.self_check()


def test_witness_preprocess_of_a_view_is_the_oracle_on_the_crop(orc):
    rng = np.random.default_rng(5)
    f = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    vs = [dict(x0=5, y0=3, w=31, h=20), dict(x0=5, y0=3, w=31, h=20, flip_x=1)]
    out = vw.preprocess_views(orc, [f], vs, 24, 40)
    assert out.shape == (2, 3, 24, 40) and out.dtype == np.float32
    assert np.array_equal(out[0:1], orc.preprocess(np.ascontiguousarray(f[3:23, 5:36]), 24, 40))
    assert np.array_equal(out[1:2], orc.preprocess(np.ascontiguousarray(f[3:23, 5:36][:, ::-1]), 24, 40))
    # mirroring commutes with the resize along x (symmetric taps, the same sums in the same order? NOT promised): only the definition
    # above is checked, and that the mirrored view differs from the plain one on this frame
    assert not np.array_equal(out[0], out[1])
    g = f.copy()
    g[vw.outside_mask((37, 53), vs)] = 255 - g[vw.outside_mask((37, 53), vs)]
    assert np.array_equal(vw.preprocess_views(orc, [g], vs, 24, 40), out)
