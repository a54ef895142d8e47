"""The proposal half of the scripts' result without a GPU: the numpy witness of run_mscnn_detection.m:75-91 (tests/proposals_witness.py)
on hand-computed rows, the pack size, the host-side refusals of mscnn_proposals_multi_fwd and the driver's proposals/<comp_id>.txt."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest

from proposals_witness import RATIOS, batch_witness, image_ranges, proposals_witness, synth_props

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hip_lib():
    L = C.CDLL(os.path.join(ROOT, "mscnn_amd/libmscnn_hip.so"))
    L.mscnn_last_error.restype = C.c_char_p
    L.mscnn_proposals_multi_pack_bytes.restype = C.c_size_t
    L.mscnn_proposals_multi_pack_bytes.argtypes = [C.c_int, C.c_int]
    L.mscnn_detections_multi_pack_bytes.restype = C.c_size_t
    L.mscnn_detections_multi_pack_bytes.argtypes = [C.c_int, C.c_int]
    L.mscnn_proposals_multi_fwd.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    return L


def test_witness_on_hand_computed_rows():
    nan, inf = float("nan"), float("inf")
    rows = np.array([
        [0, 10.5, 20.25, 110.5, 70.25, 1.5],        # kept: w 100, h 50
        [0, 10, 20, 110, 70, -10.0],                # score == proposal_thr: kept
        [0, 10, 20, 110, 70, -10.000001],           # the next float under -10: dropped
        [0, 10, 20, 110, 70, nan],                  # NaN >= thr is false
        [0, 10, 20, 110, 70, inf],                  # kept, the score stays inf
        [0, 10, 20, 110, 70, -inf],
        [0, 30, 20, 30, 70, 2.0],                   # x2 == x1 with h != 0: dropped
        [0, 30, 20, 40, 20, 2.0],                   # y2 == y1: dropped
        [0, 50, 20, 40, 70, 3.0],                   # negative width: kept (~= 0)
        [0, 0.1, 0.2, 0.4, 0.7, 0.0],               # fp32 subtraction: single(0.4) - single(0.1), not 0.3
    ], np.float32)
    assert np.float32(-10.000001) < np.float32(-10.0)
    got, keep = proposals_witness(rows, -10.0, 2.0, 4.0)
    assert keep.tolist() == [0, 1, 4, 8, 9] and keep.dtype == np.int32 and got.dtype == np.float64
    assert got[0].tolist() == [10.5 / 4, 20.25 / 2, 100.0 / 4, 50.0 / 2, 1.5]
    assert got[1].tolist() == [2.5, 10.0, 25.0, 25.0, -10.0]
    assert got[2].tolist() == [2.5, 10.0, 25.0, 25.0, inf]
    assert got[3].tolist() == [12.5, 10.0, -2.5, 25.0, 3.0]
    w32 = np.float32(0.4) - np.float32(0.1)
    h32 = np.float32(0.7) - np.float32(0.2)
    assert got[4].tolist() == [float(np.float32(0.1)) / 4, float(np.float32(0.2)) / 2, float(w32) / 4, float(h32) / 2, 0.0]
    assert float(w32) != 0.4 - 0.1      # the extent is the fp32 difference, not the double one
    # -0.0 counts as zero: x2 == x1 == -0.0 / +0.0 mixes give +-0 extents
    z = np.array([[0, -0.0, 1, 0.0, 5, 1.0], [0, 0.0, 1, -0.0, 5, 1.0]], np.float32)
    assert len(proposals_witness(z, -10.0, 1.0, 1.0)[1]) == 0


def test_witness_divides_in_double_by_the_double_ratio():
    """x / ratio with a ratio that is no fp32 number: the float64 quotient of the fp32 value, bit for bit; the fp32-division variant
    (what the final stage's boxes do) gives other bits."""
    rh, rw = RATIOS[0]
    rows = np.array([[0, 101.0, 50.0, 401.0, 250.0, 0.5]], np.float32)
    got, _ = proposals_witness(rows, -10.0, rh, rw)
    assert got[0].tolist() == [101.0 / rw, 50.0 / rh, 300.0 / rw, 200.0 / rh, 0.5]
    alt, _ = proposals_witness(rows, -10.0, rh, rw, f32_division=True)
    assert alt[0, 0] == float(np.float32(101.0) / np.float32(rw)) and alt[0, 0] != got[0, 0]


def test_batch_witness_ranges_and_empty_images():
    props = synth_props([5, 0, 3], 1)
    assert image_ranges(props, 3) == [(0, 5), (5, 0), (5, 3)]
    assert image_ranges(synth_props([0, 0, 5], 1), 3) == [(0, 0), (0, 0), (0, 5)]
    assert image_ranges(np.zeros((1, 6), np.float32), 3) == [(0, 1), (1, 0), (1, 0)]      # the whole-batch dummy row: image 0's
    out = batch_witness(props, [dict(ratios=r) for r in RATIOS])
    assert [o[2:] for o in out] == [(0, 5), (5, 0), (5, 3)] and out[1][0].shape == (0, 5)
    assert all(np.all(np.diff(k) > 0) for _, k, _, _ in out)                              # input order
    dummy = batch_witness(np.zeros((1, 6), np.float32), [dict(ratios=r) for r in RATIOS])
    assert [len(o[0]) for o in dummy] == [0, 0, 0]                                         # filtered in image 0: w == 0


def test_pack_bytes_are_the_multi_pack():
    L = hip_lib()
    for S, cap in [(1, 1), (3, 10), (8, 4800), (65, 100), (2, 0)]:
        assert L.mscnn_proposals_multi_pack_bytes(S, cap) == L.mscnn_detections_multi_pack_bytes(S, cap)
    from mscnn_amd import net as mnet
    assert mnet.detect_multi_pack_bytes(3, 1, 10) == L.mscnn_proposals_multi_pack_bytes(3, 10)


def test_op_refuses_bad_arguments_before_any_launch():
    """No device: every call below fails in the host-side checks (the fake pointers are never dereferenced) and names the value."""
    from mscnn_amd.hipapi import ProposalsDesc
    L = hip_lib()
    fake = C.c_void_p(0x1000)

    def descs(n=2, **bad):
        d = (ProposalsDesc * n)()
        for k in range(n):
            d[k].proposal_thr, d[k].ratio_h, d[k].ratio_w = -10.0, 1.5, 1.25
        for name, v in bad.items():
            setattr(d[n - 1], name, v)
        return d

    def call(d=None, n=2, props=fake, R=100, pack=fake, cap=100):
        rc = L.mscnn_proposals_multi_fwd(descs() if d is None else d, n, props, R, pack, cap, None)
        return rc, L.mscnn_last_error().decode()

    for kw in (dict(props=None), dict(pack=None)):
        rc, err = call(**kw)
        assert rc != 0 and "null pointer" in err
    rc, err = L.mscnn_proposals_multi_fwd(None, 2, fake, 100, fake, 100, None), L.mscnn_last_error().decode()
    assert rc != 0 and "null pointer" in err
    rc, err = call(n=0)
    assert rc != 0 and "0 images" in err
    rc, err = call(n=-3)
    assert rc != 0 and "-3 images" in err
    rc, err = call(R=0)
    assert rc != 0 and "R_all = 0" in err
    rc, err = call(R=100, cap=99)
    assert rc != 0 and "capacity 99 < 100 ROIs" in err
    rc, err = call(descs(ratio_h=0.0))
    assert rc != 0 and "image 1: ratios 0 x 1.25" in err
    rc, err = call(descs(ratio_w=-2.0))
    assert rc != 0 and "image 1: ratios 1.5 x -2" in err
    rc, err = call(descs(ratio_w=math.nan))
    assert rc != 0 and "image 1: ratios 1.5 x nan" in err.lower()
    rc, err = call(descs(ratio_h=math.nan))
    assert rc != 0 and "image 1: ratios nan x 1.25" in err.lower()
    rc, err = call(descs(proposal_thr=math.nan))
    assert rc != 0 and "image 1: proposal_thr is NaN" in err


def test_driver_writes_proposals_that_read_back(tmp_path):
    """tools/run_mscnn_detection.py's writer: <dir>/<comp_id>.txt, rows [image_index x y w h score] at dlmwrite's %.5g."""
    from mscnn_amd import kitti
    spec = importlib.util.spec_from_file_location("run_mscnn_detection", os.path.join(ROOT, "tools/run_mscnn_detection.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    props = synth_props([40, 0, 9], 4)
    per_image = [o[0] for o in batch_witness(props, [dict(ratios=r) for r in RATIOS])]
    assert len(per_image[0]) > 0 and len(per_image[1]) == 0 and len(per_image[2]) > 0
    out = drv.write_proposals(str(tmp_path / "proposals"), "kitti_7s_576", per_image)
    assert out == str(tmp_path / "proposals" / "kitti_7s_576.txt")
    rows = kitti.read_detections_dlm(out)
    want = [[float("%.5g" % v) for v in [i + 1] + list(p)] for i, ps in enumerate(per_image) for p in ps]
    assert rows == want and {r[0] for r in rows} == {1.0, 3.0}
    a = drv.parse_args(["--model", "kitti_car/mscnn-7s-576", "--synthetic", "2", "--proposals-out", "p", "--proposals-only"])
    assert a.proposals_only and a.proposals_out == "p"
    with pytest.raises(SystemExit):
        drv.parse_args(["--model", "kitti_car/mscnn-7s-576", "--synthetic", "2", "--proposals-only"])


def test_a_cascade_deploy_is_refused_by_name_without_a_device():
    """The refusal comes before anything touches a device: a graph-only net (device -1) shows it."""
    from mscnn_amd import net as mnet, zoo
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/cascade-mscnn-7s-576-2x", height=192, width=448, max_nms_num=200), device=-1)
    assert "proposals_score" in n.blob_names      # (the cascade deploys carry the blob: the refusal names the cascade layer)
    for call in (lambda: n.proposals_multi([dict(ratios=(1.0, 1.0))]), lambda: n.proposals_multi_device([dict(ratios=(1.0, 1.0))], 200)):
        with pytest.raises(mnet.NetError, match="cascade deploy .DecodeBBox layer proposals_2nd.*proposals_score"):
            call()
