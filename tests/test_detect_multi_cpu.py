"""The one-pass final stage's pack without a GPU: mscnn_net_unpack_detections_multi on hand-built packs (segment order, empty
segments, ids offsets, refusals) and the host-side argument checks of mscnn_detections_multi_fwd."""
import ctypes as C
import os

import numpy as np
import pytest

from mscnn_amd import net as mnet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_pack(num_classes, cap, R_all, images, counts, hdr3=0):
    """images: [(row0, rows)] per image; counts[image * C + class].  Segment (i, c) owns pack rows [C row0 + c rows, + rows):
    det row k of it = [s, k, row0, rows, 100 s + k], id = k (relative to row0)."""
    B = len(images)
    S = B * num_classes
    nbytes = mnet.detect_multi_pack_bytes(B, num_classes, cap)
    buf = np.zeros(nbytes, np.uint8)
    words = buf[:16 * (S + 1)].view(np.int32).reshape(S + 1, 4)
    words[0] = [S, R_all, cap, hdr3]
    table = 16 * (S + 1)
    dets = buf[table:table + 40 * max(cap, 1)].view(np.float64).reshape(-1, 5)
    ids = buf[table + 40 * max(cap, 1):table + 44 * max(cap, 1)].view(np.int32)
    dets[:] = -7.0
    ids[:] = -7
    for s in range(B * num_classes):
        i, c = divmod(s, num_classes)
        row0, rows = images[i]
        words[1 + s] = [counts[s], rows, row0, 0]
        slot = num_classes * row0 + c * rows
        for k in range(max(counts[s], 0)):
            dets[slot + k] = [s, k, row0, rows, 100 * s + k]
            ids[slot + k] = k
    return buf


def test_pack_bytes_match_the_op_library():
    L = C.CDLL(os.path.join(ROOT, "mscnn_amd/libmscnn_hip.so"))
    L.mscnn_detections_multi_pack_bytes.restype = C.c_size_t
    for B, Cn, cap in [(1, 1, 1), (2, 2, 10), (8, 2, 4800), (3, 3, 0)]:
        got = mnet.detect_multi_pack_bytes(B, Cn, cap)
        assert got == L.mscnn_detections_multi_pack_bytes(B * Cn, cap)
        assert got % 16 == 0 and got >= 16 * (B * Cn + 1) + 44 * max(cap, 1)


def test_segment_order_and_ids_offsets():
    images = [(0, 3), (3, 2), (5, 4)]           # three images, rows grouped by image
    counts = [2, 3, 1, 0, 4, 1]                 # (image, class) image-major, two classes
    pack = make_pack(2, 18, 9, images, counts)
    segs, rois = mnet.unpack_detections_multi(pack, 3, 2, 18)
    assert rois == [3, 2, 4]
    for i, (row0, rows) in enumerate(images):
        for c in range(2):
            s = 2 * i + c
            dets, ids = segs[i][c]
            assert dets.shape == (counts[s], 5)
            assert np.array_equal(dets[:, 0], np.full(counts[s], s))                 # from this segment's own slot
            assert np.array_equal(dets[:, 4], 100 * s + np.arange(counts[s]))        # in the slot's order
            assert np.array_equal(ids, row0 + np.arange(counts[s]))                  # rows of the net's ROI blobs


def test_empty_segments_and_images_without_rows():
    # the whole-batch dummy row: image 0 owns row 0, every other image none
    pack = make_pack(3, 3, 1, [(0, 1), (1, 0), (1, 0)], [0] * 9)
    segs, rois = mnet.unpack_detections_multi(pack, 3, 3, 3)
    assert rois == [1, 0, 0]
    assert all(d.shape == (0, 5) and i.shape == (0,) for row in segs for d, i in row)
    pack = make_pack(1, 4, 4, [(0, 4)], [1])
    segs, rois = mnet.unpack_detections_multi(pack, 1, 1, 4)
    assert rois == [4] and len(segs[0][0][0]) == 1


def test_out_capacity_overflow_is_refused_with_the_numbers():
    pack = make_pack(2, 12, 6, [(0, 4), (4, 2)], [3, 2, 1, 1])
    segs, _ = mnet.unpack_detections_multi(pack, 2, 2, 12, out_cap=7)
    assert sum(len(d) for row in segs for d, _ in row) == 7
    with pytest.raises(mnet.NetError, match="holds 6 rows.*have 7"):
        mnet.unpack_detections_multi(pack, 2, 2, 12, out_cap=6)


@pytest.mark.parametrize("case,match", [
    ("segments", "another number of segments"),
    ("cap", "another capacity"),
    ("r_all", "corrupt detection pack header"),
    ("hdr3", "corrupt detection pack header"),
    ("count_over_rows", "corrupt detection pack: segment 1"),
    ("rows_past_end", "corrupt detection pack: segment 2"),
    ("disagree", "disagree on its rows"),
    ("over_bound", "more than the per-image row bound"),
])
def test_corrupt_or_foreign_packs_are_refused(case, match):
    images, counts, B, Cn, cap = [(0, 4), (4, 2)], [1, 2, 0, 1], 2, 2, 12
    if case == "r_all":
        pack = make_pack(Cn, cap, 7, images, counts)           # 2 x 7 rows do not fit a 12-row pack
    elif case == "hdr3":
        pack = make_pack(Cn, cap, 6, images, counts, hdr3=5)
    else:
        pack = make_pack(Cn, cap, 6, images, counts)
    w = pack[:16 * (B * Cn + 1)].view(np.int32).reshape(-1, 4)
    if case == "segments":
        w[0, 0] = 3
    elif case == "count_over_rows":
        w[2, 0] = 5                                             # segment 1 = image 0 (4 rows), 5 detections
    elif case == "rows_past_end":
        w[3, 1] = 3; w[4, 1] = 3                                # image 1: rows [4, 7) of 6
    elif case == "disagree":
        w[4, 2] = 3                                             # class 1 of image 1 names another row0
    elif case == "over_bound":
        w[3, 0] = -1
    with pytest.raises(mnet.NetError, match=match):
        mnet.unpack_detections_multi(pack, B, Cn, cap - 1 if case == "cap" else cap)


def test_op_refuses_bad_arguments_before_any_launch():
    """mscnn_detections_multi_fwd's host-side checks (no device pointer is dereferenced: every call fails before a launch)."""
    L = C.CDLL(os.path.join(ROOT, "mscnn_amd/libmscnn_hip.so"))
    L.mscnn_last_error.restype = C.c_char_p
    L.mscnn_detections_multi_workspace_bytes.restype = C.c_size_t
    L.mscnn_detections_multi_workspace_bytes.argtypes = [C.c_int, C.c_int]
    L.mscnn_detections_multi_fwd.argtypes = ([C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p, C.c_int,
                                             C.c_void_p, C.c_size_t, C.c_void_p])
    assert L.mscnn_detections_multi_workspace_bytes(4, 4033) == 0
    assert L.mscnn_detections_multi_workspace_bytes(4, 300) > 0
    from mscnn_amd.hipapi import DetectionsDesc
    descs = (DetectionsDesc * 4)()
    for d in descs:
        d.ncls, d.cls_id = 3, 2
    fake = C.c_void_p(0x1000)      # never touched: every case below is refused first

    def call(R_all, max_rows, cap):
        rc = L.mscnn_detections_multi_fwd(descs, 2, 2, fake, fake, fake, R_all, max_rows, fake, cap, fake, C.c_size_t(1 << 40), None)
        return rc, L.mscnn_last_error().decode()

    rc, err = call(100, 4033, 200)
    assert rc != 0 and "4033 rows per image > 4032" in err
    rc, err = call(100, 60, 199)
    assert rc != 0 and "capacity 199 < 2 classes x 100 ROIs" in err
    descs[3].cls_id = 4
    rc, err = call(100, 60, 200)
    assert rc != 0 and "segment 3: cls_id 4 of 3" in err
