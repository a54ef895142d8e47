"""Caller-supplied ROIs without a GPU: the exports and ctypes prototypes of mscnn_rois_ingest_f32 / mscnn_net_forward_rois, the
host-side refusals of the op (nothing is launched: the fake pointers are never dereferenced), the refusal of a graph-only net, the
layers forward_rois runs around, and the driver's --rois-in parser."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def driver():
    spec = importlib.util.spec_from_file_location("run_mscnn_detection", os.path.join(ROOT, "tools/run_mscnn_detection.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    return drv


def test_exports_and_prototypes():
    from mscnn_amd import hipapi, net as mnet
    L = hipapi.lib()
    assert L.mscnn_rois_ingest_f32.argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 7
    assert L.mscnn_rois_reason_text.restype is C.c_char_p
    assert (hipapi.ROIS_NET, hipapi.ROIS_IMAGE) == (0, 1)
    assert (hipapi.ROIS_BAD_NONFINITE, hipapi.ROIS_BAD_IMAGE, hipapi.ROIS_BAD_ORDER) == (1, 2, 3)
    texts = [L.mscnn_rois_reason_text(r).decode() for r in (1, 2, 3)]
    assert "finite" in texts[0] and "image index" in texts[1] and "grouped by image" in texts[2]
    N = mnet.lib()
    assert N.mscnn_net_forward_rois.argtypes == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    assert N.mscnn_net_forward_rois_layers.argtypes == [C.c_void_p] * 3
    assert callable(mnet.Net.forward_rois)
    header = open(os.path.join(ROOT, "include/mscnn_hip.h")).read()
    for formula in ("x1 = (float)(x * ratio_w)", "x2 = (float)((x + w) * ratio_w)", "y1 = (float)(y * ratio_h)",
                    "y2 = (float)((y + h) * ratio_h)"):
        assert formula in header, formula


def test_op_refuses_bad_arguments_before_any_launch():
    from mscnn_amd import hipapi
    L = hipapi.lib()
    fake = C.c_void_p(0x1000)
    ones = (C.c_double * 2)(1.5, 1.25)

    def call(rows=fake, coords=0, R=10, N=2, rh=None, rw=None, rois=fake, props=fake, image_rows=fake, status=fake):
        rc = L.mscnn_rois_ingest_f32(rows, coords, R, N, rh, rw, rois, props, image_rows, status, None)
        return rc, L.mscnn_last_error().decode()

    for name in ("rows", "rois", "image_rows", "status"):
        rc, err = call(**{name: None})
        assert rc != 0 and "null pointer" in err and name in err, (name, err)
    rc, err = call(R=0)
    assert rc != 0 and "R = 0" in err
    rc, err = call(R=-4)
    assert rc != 0 and "R = -4" in err
    rc, err = call(N=0)
    assert rc != 0 and "N = 0" in err
    rc, err = call(coords=2)
    assert rc != 0 and "coords = 2" in err
    rc, err = call(rows=C.c_void_p(0x1004))
    assert rc != 0 and "rows must be 8-byte aligned" in err
    rc, err = call(coords=1, rows=C.c_void_p(0x1004), rh=ones, rw=ones)
    assert rc != 0 and "rows must be 8-byte aligned" in err
    for name in ("rois", "props", "image_rows", "status"):
        rc, err = call(**{name: C.c_void_p(0x1002)})
        assert rc != 0 and f"{name} must be 4-byte aligned" in err, (name, err)
    # the original-image form: ratios are part of the call
    rc, err = call(coords=1)
    assert rc != 0 and "null pointer" in err and "ratio_h" in err
    rc, err = call(coords=1, N=hipapi.ROIS_MAX_RATIO_IMAGES + 1, rh=ones, rw=ones)
    assert rc != 0 and f"N = {hipapi.ROIS_MAX_RATIO_IMAGES + 1}" in err
    for bad, text in ((0.0, "0 x 1.25"), (-2.0, "-2 x 1.25"), (math.nan, "nan x 1.25"), (math.inf, "inf x 1.25")):
        rc, err = call(coords=1, rh=(C.c_double * 2)(1.5, bad), rw=ones)
        assert rc != 0 and f"image 1: ratios {text}" in err.lower(), err


def test_a_graph_only_net_is_refused_naming_the_device():
    from mscnn_amd import net as mnet, zoo
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=96, width=320, max_nms_num=120), device=-1)
    with pytest.raises(mnet.NetError, match="forward_rois: the net was built with device -1"):
        n.forward_rois(np.array([[0, 1, 2, 30, 40, 0.5]], np.float32))
    with pytest.raises(mnet.NetError, match="device -1"):
        n.forward_rois(np.array([[0, 1, 2, 30, 40, 0.5]], np.float64), "image", [dict(ratios=(1.0, 1.0))])
    with pytest.raises(mnet.NetError, match="coords 'pixels'"):
        n.forward_rois(np.zeros((1, 6), np.float32), "pixels")
    with pytest.raises(mnet.NetError, match=r"rows must be \[R, 6\]"):
        n.forward_rois(np.zeros((4, 5), np.float32))


@pytest.mark.parametrize("model,size", [
    ("kitti_car/mscnn-7s-576", dict(height=96, width=320, max_nms_num=120)),
    ("kitti_ped_cyc/mscnn-7s-576-2x", dict(height=192, width=448, max_nms_num=200)),
    ("caltech/mscnn-7s-480", dict(height=240, width=320, max_nms_num=150)),
    ("kitti_car/cascade-mscnn-7s-576-2x", dict(height=192, width=448, max_nms_num=150)),
    ("widerface/cascade-mscnn-12s-align", dict(height=160, width=192, max_nms_num=150)),
])
def test_the_layers_forward_rois_runs_around(model, size):
    """L is the BoxOutput layer that writes proposals_score; K is the Split the graph builder puts behind relu4_3 (conv4_3 has several
    readers); conv5_x, the proposal heads and BoxOutput lie between them, the "-2x" nets' Deconvolution behind L."""
    from mscnn_amd import net as mnet, zoo
    n = mnet.Net(prototxt_text=zoo.prototxt(model, **size), device=-1)
    L, K = n.forward_rois_layers()
    assert n.layer_types[L] == "BoxOutput" and n.layer_tops(L)[1] == "proposals_score"
    assert n.layer_types[K] == "Split" and n.layer_names[K - 1] == "relu4_3" and K < L
    between = n.layer_names[K + 1:L]
    assert any(nm.startswith("LFCN_") for nm in between)
    deeper = [nm for nm in n.layer_names if nm.startswith(("conv5_", "conv6_", "pool6"))]
    assert deeper and set(deeper) <= set(between)
    assert not any(t in ("ROIPooling", "ROIAlign") for t in n.layer_types[:L])
    if "conv4_3_2x" in n.blob_names:
        assert n.layer_types.index("Deconvolution") > L


def test_a_net_without_roi_layers_is_refused():
    from mscnn_amd import net as mnet
    text = """
    name: "plain"
    input: "data" input_shape { dim: 1 dim: 3 dim: 16 dim: 16 }
    layer { name: "c" type: "Convolution" bottom: "data" top: "c" convolution_param { num_output: 4 kernel_size: 3 pad: 1 } }
    """
    n = mnet.Net(prototxt_text=text, device=-1)
    with pytest.raises(mnet.NetError, match="no ROIPooling / ROIAlign layer"):
        n.forward_rois_layers()


def test_rois_in_parser(tmp_path):
    from mscnn_amd import kitti
    drv = driver()
    per_image = [np.array([[10.5, 20.25, 100.0, 50.0, 0.75], [1, 2, 3, 4, -2.5]]), np.zeros((0, 5)), np.array([[7, 8, 9, 10, 0.125]])]
    path = str(tmp_path / "rois.txt")
    kitti.write_detections_dlm(path, per_image)                     # the writer of --proposals-out: 1-based indices 1 and 3
    assert [r[0] for r in kitti.read_detections_dlm(path)] == [1.0, 1.0, 3.0]
    got = drv.read_rois(path, 4)
    assert [len(g) for g in got] == [2, 0, 1, 0]                    # an image without rows: 0 rows, also behind the last index
    assert all(g.dtype == np.float64 and g.shape[1] == 5 for g in got)
    assert np.array_equal(got[0], per_image[0]) and np.array_equal(got[2], per_image[2])
    rows = drv.group_rois(got[:3])
    assert rows.dtype == np.float64 and rows.shape == (3, 6) and rows[:, 0].tolist() == [0.0, 0.0, 2.0]      # 0-based inside the group
    assert np.array_equal(rows[:, 1:], np.concatenate([per_image[0], per_image[2]]))
    assert drv.group_rois(got[2:3])[:, 0].tolist() == [0.0]
    # refusals
    with open(path, "w") as f:
        f.write("2,1,2,3,4,0.5\n1,1,2,3,4,0.5\n")
    with pytest.raises(ValueError, match="row 2: image index 1 after 2"):
        drv.read_rois(path, 3)
    with open(path, "w") as f:
        f.write("0,1,2,3,4,0.5\n")
    with pytest.raises(ValueError, match="image index 0 outside 1 .. 3"):
        drv.read_rois(path, 3)
    with open(path, "w") as f:
        f.write("4,1,2,3,4,0.5\n")
    with pytest.raises(ValueError, match="image index 4 outside 1 .. 3"):
        drv.read_rois(path, 3)
    with open(path, "w") as f:
        f.write("1,1,2,3,4\n")
    with pytest.raises(ValueError, match="row 1 has 5 values"):
        drv.read_rois(path, 3)
    # the switches
    a = drv.parse_args(["--model", "kitti_car/mscnn-7s-576", "--synthetic", "2", "--rois-in", path])
    assert a.rois_in == path and not a.proposals_only
    with pytest.raises(SystemExit):
        drv.parse_args(["--model", "kitti_car/mscnn-7s-576", "--synthetic", "2", "--rois-in", path, "--proposals-out", "p", "--proposals-only"])
