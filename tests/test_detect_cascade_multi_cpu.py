"""The one-pass cascade final stage without a GPU: the pack of mscnn_net_detect_cascade_multi (K = outputs x classes slots per
image) on hand-built packs, the host-side refusals of mscnn_detections_cascade_multi_fwd and of the net call (graph-only net: no
HIP device is touched), and the --orig-size rule and argument checks of tools/run_cascademscnn.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from mscnn_amd import net as mnet, zoo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(1, os.path.join(ROOT, "tools"))


def make_pack(O, Cn, cap, R_all, images, counts):
    """images: [(row0, rows)] per image; counts[(image * O + output) * C + class].  Segment (i, o, c) owns pack rows
    [K row0 + (o C + c) rows, + rows), K = O C: det row k of it = [i, o, c, k, 100 s + k], id = k (relative to row0)."""
    B, K = len(images), O * Cn
    S = B * K
    buf = np.zeros(mnet.detect_cascade_multi_pack_bytes(B, O, Cn, cap), np.uint8)
    words = buf[:16 * (S + 1)].view(np.int32).reshape(S + 1, 4)
    words[0] = [S, R_all, cap, 0]
    table = 16 * (S + 1)
    dets = buf[table:table + 40 * max(cap, 1)].view(np.float64).reshape(-1, 5)
    ids = buf[table + 40 * max(cap, 1):table + 44 * max(cap, 1)].view(np.int32)
    dets[:] = -7.0
    ids[:] = -7
    for s in range(S):
        i, k = divmod(s, K)
        o, c = divmod(k, Cn)
        row0, rows = images[i]
        words[1 + s] = [counts[s], rows, row0, 0]
        slot = K * row0 + k * rows
        for j in range(max(counts[s], 0)):
            dets[slot + j] = [i, o, c, j, 100 * s + j]
            ids[slot + j] = j
    return buf


def test_pack_bytes_match_the_op_library():
    L = C.CDLL(os.path.join(ROOT, "mscnn_amd/libmscnn_hip.so"))
    L.mscnn_detections_multi_pack_bytes.restype = C.c_size_t
    for B, O, Cn, cap in [(1, 1, 1, 1), (2, 3, 2, 60), (4, 3, 3, 5400), (3, 4, 1, 0)]:
        got = mnet.detect_cascade_multi_pack_bytes(B, O, Cn, cap)
        assert got == L.mscnn_detections_multi_pack_bytes(B * O * Cn, cap)
        assert got % 16 == 0 and got >= 16 * (B * O * Cn + 1) + 44 * max(cap, 1)


def test_hand_built_pack_unpacks_image_then_output_then_class():
    images = [(0, 3), (3, 0), (3, 2)]                    # the middle image owns no rows
    O, Cn = 3, 2
    counts = [2, 3, 1, 0, 3, 1,  0, 0, 0, 0, 0, 0,  2, 1, 0, 2, 1, 1]
    pack = make_pack(O, Cn, 30, 5, images, counts)
    per_image, rois = mnet.unpack_detections_cascade_multi(pack, 3, O, Cn, 30)
    assert rois == [3, 0, 2]
    assert len(per_image) == 3 and all(len(r) == O and all(len(q) == Cn for q in r) for r in per_image)
    for i, (row0, rows) in enumerate(images):
        for o in range(O):
            for c in range(Cn):
                s = (i * O + o) * Cn + c
                dets, ids = per_image[i][o][c]
                assert dets.shape == (counts[s], 5)
                assert np.array_equal(dets[:, :3], np.tile([i, o, c], (counts[s], 1)))      # from this segment's own slot
                assert np.array_equal(dets[:, 4], 100 * s + np.arange(counts[s]))           # in the slot's order
                assert np.array_equal(ids, row0 + np.arange(counts[s]))                     # rows of the net's blobs
    w = pack[:16 * (3 * O * Cn + 1)].view(np.int32).reshape(-1, 4)
    w[1 + 13, 0] = -1                                    # a segment of image 2 over the per-image bound
    with pytest.raises(mnet.NetError, match="image 2 has 2 ROIs, more than the per-image row bound"):
        mnet.unpack_detections_cascade_multi(pack, 3, O, Cn, 30)


def _op():
    from mscnn_amd.hipapi import CascadeOutput, DetectionsDesc
    L = C.CDLL(os.path.join(ROOT, "mscnn_amd/libmscnn_hip.so"))
    L.mscnn_last_error.restype = C.c_char_p
    L.mscnn_detections_cascade_multi_workspace_bytes.restype = C.c_size_t
    L.mscnn_detections_cascade_multi_workspace_bytes.argtypes = [C.c_int, C.c_int]
    L.mscnn_detections_cascade_multi_fwd.argtypes = ([C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                     C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p])
    return L, CascadeOutput, DetectionsDesc


def test_op_refuses_bad_arguments_before_any_launch():
    """mscnn_detections_cascade_multi_fwd's host-side checks (no device pointer is dereferenced: every call fails before a launch)."""
    L, CascadeOutput, DetectionsDesc = _op()
    assert L.mscnn_detections_cascade_multi_workspace_bytes(12, 4033) == 0
    assert L.mscnn_detections_cascade_multi_workspace_bytes(12, 300) > 0
    B, Cn = 2, 2
    fake = 0x1000                  # never touched: every case below is refused first

    def call(O, R_all=100, max_rows=60, cap=None, cls=(2, 2), null=None, ncls=(3, 3, 2, 3, 3)):
        n = max(O, 1)
        outs = (CascadeOutput * max(n, 5))()
        for o in range(max(n, 5)):
            outs[o].boxes, outs[o].cls_prob, outs[o].props, outs[o].ncls = fake, fake, fake, ncls[o]
        if null is not None:
            setattr(outs[null[0]], null[1], None)
        descs = (DetectionsDesc * (B * n * Cn))()
        for s, d in enumerate(descs):
            d.ncls, d.cls_id = 3, cls[s % Cn]
        rc = L.mscnn_detections_cascade_multi_fwd(descs, 0.0, B, O, Cn, outs, R_all, max_rows, C.c_void_p(fake),
                                                  O * Cn * R_all if cap is None else cap, C.c_void_p(fake), C.c_size_t(1 << 40), None)
        return rc, L.mscnn_last_error().decode()

    rc, err = call(0)
    assert rc != 0 and "0 cascade outputs (1 .. 4)" in err, err
    rc, err = call(5)
    assert rc != 0 and "5 cascade outputs (1 .. 4)" in err, err
    for field in ("boxes", "cls_prob", "props"):
        rc, err = call(3, null=(1, field))
        assert rc != 0 and "output 1 of 3: null pointer" in err, err
    rc, err = call(3, cls=(2, 3))                       # output 2 has two probability columns: segment (0, 2, 1) asks for the third
    assert rc != 0 and "segment 5 (output 2): cls_id 3 of 2" in err, err
    rc, err = call(3, cls=(0, 2))
    assert rc != 0 and "segment 0 (output 0): cls_id 0 of 3" in err, err
    rc, err = call(3, cap=599)
    assert rc != 0 and "capacity 599 < 3 outputs x 2 classes x 100 ROIs" in err, err
    rc, err = call(3, max_rows=4033)
    assert rc != 0 and "4033 rows per image > 4032" in err, err
    rc, err = call(3, R_all=0)
    assert rc != 0 and "R_all = 0" in err, err


TRIPLES = [("output_bbox_1st", "cls_prob_1st", "proposals"), ("output_bbox_2nd", "cls_prob_2nd", "proposals_2nd"),
           ("output_bbox_3rd", "cls_prob_3rd", "proposals_3rd")]


def test_net_call_refuses_bad_arguments_before_touching_the_device():
    """mscnn_net_detect_cascade_multi / _device on a graph-only net (device -1: no HIP device is touched, so every case is refused
    before a reservation or a launch)."""
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/cascade-mscnn-7s-576-2x", height=192, width=448, max_nms_num=150, batch=2),
                 device=-1)
    kw = dict(ratios=(0.5, 0.4), org_hw=(375, 1242))
    R = n.blob_shape("proposals")[0]
    ncls = n.blob_shape("cls_prob_1st")[1]
    assert ncls == 5 and R >= 1
    with pytest.raises(mnet.NetError, match=r"0 cascade outputs \(1 \.\. 4\)"):
        n.detect_cascade_multi([kw] * 2, [], [2])
    with pytest.raises(mnet.NetError, match=r"5 cascade outputs \(1 \.\. 4\)"):
        n.detect_cascade_multi([kw] * 2, TRIPLES + TRIPLES[:2], [2])
    with pytest.raises(mnet.NetError, match="output 1 of 2: null blob name"):
        n.detect_cascade_multi([kw] * 2, [TRIPLES[0], ("output_bbox_2nd", None, "proposals_2nd")], [2], cap=10)
    with pytest.raises(mnet.NetError, match=r"Unknown blob name cls_prob_4th \(cascade output 1\)"):
        n.detect_cascade_multi([kw] * 2, [TRIPLES[0], ("output_bbox_2nd", "cls_prob_4th", "proposals_2nd")], [2], cap=10)
    with pytest.raises(mnet.NetError, match=rf"bbox_pred is not an \[R, 5\] box blob \({8 * R} values in {R} rows\)"):
        n.detect_cascade_multi([kw] * 2, [("bbox_pred", "cls_prob_1st", "proposals")], [2])
    with pytest.raises(mnet.NetError, match=rf"proposals_score is not an \[R, 5\] proposal blob \({6 * R} values in {R} rows\)"):
        n.detect_cascade_multi([kw] * 2, [("output_bbox_1st", "cls_prob_1st", "proposals_score")], [2])
    d = n.blob_shape("data")[0]
    with pytest.raises(mnet.NetError, match=rf"cascade output 0: output_bbox_1st has {R} rows, data {d}, proposals {R}"):
        n.detect_cascade_multi([kw] * 2, [("output_bbox_1st", "data", "proposals")], [2])
    with pytest.raises(mnet.NetError, match=rf"segment 1 \(output 0\): cls_id {ncls + 1} of {ncls}"):
        n.detect_cascade_multi([kw] * 2, TRIPLES, [2, ncls + 1])
    with pytest.raises(mnet.NetError, match=rf"segment 0 \(output 0\): cls_id 0 of {ncls}"):
        n.detect_cascade_multi([kw] * 2, TRIPLES[:1], [0])
    with pytest.raises(mnet.NetError, match="num_images 3 but the net's input holds 2 images"):
        n.detect_cascade_multi([kw] * 3, TRIPLES, [2])
    with pytest.raises(mnet.NetError, match=rf"capacity {6 * R - 1} < 3 outputs x 2 classes x {R} ROIs"):
        n.detect_cascade_multi_device([kw] * 2, TRIPLES, [2, 3], 6 * R - 1)


def test_orig_size_rule():
    """widerface/run_cascademscnn.m:82-91 by hand: round(x / 32) * 32 with MATLAB's round (halves away from zero); over max_size on
    either side, both sides times max_size / the larger rounded side, rounded with the same rule."""
    from run_cascademscnn import matlab_round, net_input_size
    assert [matlab_round(v) for v in (22.5, 23.5, 0.5, 22.49, -2.5)] == [23, 24, 1, 22, -3]
    assert net_input_size(720, 1024) == (736, 1024)           # 720 / 32 = 22.5 -> 23 (Python's round gives 22 -> 704)
    assert net_input_size(600, 720) == (608, 736)             # 18.75 -> 19; 22.5 -> 23
    assert net_input_size(1024, 2048) == (1024, 2048)         # multiples of 32 stay
    assert net_input_size(3072, 3072) == (3072, 3072)         # at max_size: not scaled
    # 4000 x 3000: 125 -> 4000, 93.75 -> 94 -> 3008; t = 3072 / 4000 = 0.768: 4000 t / 32 = 96 -> 3072, 3008 t / 32 = 72.192 -> 2304
    assert net_input_size(4000, 3000) == (3072, 2304)
    # 1000 x 5000 at max_size 1280: 31.25 -> 992, 156.25 -> 4992; t = 1280 / 4992: 992 t / 32 = 7.9487 -> 256, 4992 t / 32 = 40 -> 1280
    assert net_input_size(1000, 5000, max_size=1280) == (256, 1280)
    # a half-way case AFTER scaling: 2000 x 1200 at max_size 1000: 62.5 -> 63 -> 2016, 37.5 -> 38 -> 1216; t = 1000 / 2016:
    # 2016 t / 32 = 31.25 -> 992, 1216 t / 32 = 18.849 -> 608
    assert net_input_size(2000, 1200, max_size=1000) == (992, 608)


def test_driver_refuses_batch_with_orig_size_without_a_gpu():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools/run_cascademscnn.py"), "--model", "widerface/cascade-mscnn-12s-align",
                        "--synthetic", "2", "--batch", "2", "--orig-size"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert "--orig-size with --batch 2" in r.stderr and "one frame per forward" in r.stderr, r.stderr
    from run_cascademscnn import default_outputs, parse_args
    a = parse_args(["--model", "kitti_car/cascade-mscnn-7s-576-2x", "--synthetic", "4", "--batch", "2", "--outputs", "1st,2nd,3rd"])
    assert a.batch == 2 and a.outputs == "1st,2nd,3rd" and not a.orig_size
    assert default_outputs(["proposals", "proposals_3rd", "cls_prob_3rd"]) == ["3rd"]
    assert default_outputs(["proposals", "proposals_3rd", "cls_prob_3rd", "cls_prob_3rd_avg"]) == ["3rd_avg"]
    assert default_outputs(["proposals", "cls_prob_1st"]) == ["1st"]
    with pytest.raises(SystemExit):
        parse_args(["--model", "kitti_car/cascade-mscnn-7s-576-2x", "--synthetic", "1", "--outputs", "4th"])
