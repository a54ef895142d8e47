"""The one-pass final stage on the GPU: mscnn_detections_multi_fwd against mscnn_detections_fwd on every segment's row range (bit for
bit, ids included) and against the oracle (selection-exact), and mscnn_net_detect_multi / _device against the per-call stages of
batched nets (bit for bit)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from mscnn_amd import net as mnet, synth, zoo   # noqa: E402

NCLS = 4


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X: torch.cuda.is_available() is False")
    from mscnn_amd import hipapi
    hipapi.lib()
    return hipapi


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rel_err(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return 0.0 if a.size == 0 else float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())


def batch_rois(rows_per_image, seed, all_filtered=()):
    """ROI blobs of a batch grouped by image (column 0 of props = image index): clustered boxes, some rows below proposal_thr, some
    with zero width, exact probability ties; images in all_filtered have every row under proposal_thr."""
    rng = np.random.default_rng(seed)
    parts = []
    for i, n in enumerate(rows_per_image):
        c = rng.uniform(0, 1500, (max(1, n // 12), 2))
        xy = c[rng.integers(0, len(c), n)] + rng.normal(0, 12, (n, 2))
        wh = rng.uniform(20, 200, (n, 2))
        sc = rng.normal(0, 4, (n, 1))
        if i in all_filtered:
            sc[:] = -11.0
        parts.append(np.concatenate([np.full((n, 1), i), xy, xy + wh, sc], 1).astype(np.float32))
    props = np.concatenate(parts, 0)
    R = len(props)
    props[::17, 5] = np.minimum(props[::17, 5], -11.0)
    props[5::29, 3] = props[5::29, 1]
    bbox_pred = rng.standard_normal((R, 4 * NCLS)).astype(np.float32)
    cls_pred = (rng.standard_normal((R, NCLS)) * 2).astype(np.float32)
    cls_pred[3::7] = cls_pred[2::7][: len(cls_pred[3::7])]
    return bbox_pred, cls_pred, props


def image_kw(i):
    org = (375 + 40 * i, 1242 - 60 * i)
    return dict(ratios=(576 / org[0], 1920 / org[1]), org_hw=org, nms_overlap=0.5 if i % 2 == 0 else 0.6)


def check_op(hip, orc, bbox_pred, cls_pred, props, num_images, classes, max_rows=None):
    segs = [dict(cls_id=c, **image_kw(i)) for i in range(num_images) for c in classes]
    out = hip.detections_multi(dev(bbox_pred), dev(cls_pred), dev(props), num_images, segs, max_rows)
    img = props[:, 0].astype(int)
    total = 0
    for s, (dets, ids, row0, rows) in enumerate(out):
        i = s // len(classes)
        r = np.flatnonzero(img == i)
        want0, wantn = (int(r[0]), len(r)) if len(r) else (int(np.searchsorted(img, i)), 0)
        assert (row0, rows) == (want0, wantn), (s, row0, rows)
        sl = slice(row0, row0 + rows)
        d1, i1 = hip.detections(dev(bbox_pred[sl]), dev(cls_pred[sl]), dev(props[sl]), **segs[s])
        assert np.array_equal(ids, i1.cpu().numpy()), s                    # the per-call stage on the range: bit for bit
        assert np.array_equal(dets.view(np.uint64), d1.cpu().numpy().view(np.uint64)), s
        dref, iref = orc.detections(bbox_pred[sl], cls_pred[sl], props[sl], **segs[s])
        assert np.array_equal(ids, iref), s                                  # selection + order against the oracle
        assert rel_err(dets, dref) < 1e-4, s
        total += len(dets)
    return out, total


@pytest.mark.parametrize("classes", [[2, 3], [2, 3, 4]])
def test_multi_op_every_segment_equals_the_per_range_stage(hip, orc, classes):
    rows = [1, 63, 0, 64, 65, 300, 40, 7]          # image 2 has no rows, image 6's rows are all under proposal_thr
    bbox_pred, cls_pred, props = batch_rois(rows, 11 + len(classes), all_filtered=(6,))
    out, total = check_op(hip, orc, bbox_pred, cls_pred, props, len(rows), classes, max_rows=max(rows))
    assert total > 0
    assert all(len(out[6 * len(classes) + c][0]) == 0 for c in range(len(classes)))
    if len(classes) == 2:                          # the loosest host bound: every row of the batch
        check_op(hip, orc, bbox_pred, cls_pred, props, len(rows), classes)


def test_multi_op_whole_batch_dummy_row_and_segment_chunks(hip, orc):
    """The [0 0 0 0 0 0] row BoxOutput emits when nothing survives in the whole batch (image 0 owns it, the others own nothing), and a
    batch of more segments than one launch carries (3 launches of up to 32)."""
    z = np.zeros((1, 6), np.float32)
    out, total = check_op(hip, orc, np.zeros((1, 4 * NCLS), np.float32), np.zeros((1, NCLS), np.float32), z, 3, [2, 3])
    assert total == 0 and [o[3] for o in out] == [1, 1, 0, 0, 0, 0]
    rows = [5, 0, 70] * 12                          # 36 images x 2 classes = 72 segments
    bbox_pred, cls_pred, props = batch_rois(rows, 5)
    check_op(hip, orc, bbox_pred, cls_pred, props, len(rows), [2, 3], max_rows=70)


def test_multi_op_mask_word_boundary_empty_image_and_an_image_over_the_bound(hip, orc):
    """Images of 64, 0 and 65 rows (both sides of a 64-bit mask word, nothing in between), classes [2, 3], through the one-source
    path; then the same inputs with max_rows_per_image = 64: the segments of the 65-row image come back as over the bound (count -1:
    (None, None, row0, rows)), every other segment unchanged."""
    rows, classes = [64, 0, 65], [2, 3]
    bbox_pred, cls_pred, props = batch_rois(rows, 23)
    # not vacuous, on the oracle's output: every non-empty segment has a detection and a suppressed box
    passed = (props[:, 5] >= -10.0) & (props[:, 3] - props[:, 1] != 0) & (props[:, 4] - props[:, 2] != 0)
    for i, sl in ((0, slice(0, 64)), (2, slice(64, 129))):
        for c in classes:
            dref, _ = orc.detections(bbox_pred[sl], cls_pred[sl], props[sl], cls_id=c, **image_kw(i))
            assert 0 < len(dref) < int(passed[sl].sum()), (i, c)
    out, _ = check_op(hip, orc, bbox_pred, cls_pred, props, 3, classes, max_rows=65)
    assert [(o[2], o[3]) for o in out] == [(0, 64)] * 2 + [(64, 0)] * 2 + [(64, 65)] * 2
    segs = [dict(cls_id=c, **image_kw(i)) for i in range(3) for c in classes]
    over = hip.detections_multi(dev(bbox_pred), dev(cls_pred), dev(props), 3, segs, 64)
    assert over[4:] == [(None, None, 64, 65)] * 2
    for a, b in zip(over[:4], out[:4]):
        assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


# ---- the net entries ---------------------------------------------------------------------------------------------------------------
NETS = [   # model, reduced input, batch, classes
    ("kitti_car/mscnn-7s-576", dict(height=96, width=320, max_nms_num=120), 4, [2]),
    ("caltech/mscnn-7s-480", dict(height=240, width=320, max_nms_num=150), 2, [2]),
    ("kitti_ped_cyc/mscnn-7s-576-2x", dict(height=192, width=448, max_nms_num=200), 2, [2, 3]),
]


def _pack_to_host(ptr, nbytes):
    torch.cuda.synchronize()
    hiprt = C.CDLL("libamdhip64.so")
    host = np.zeros(nbytes, np.uint8)
    assert hiprt.hipDeviceSynchronize() == 0
    assert hiprt.hipMemcpy(host.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(nbytes), 2) == 0      # hipMemcpyDeviceToHost
    return host


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("model,size,batch,classes", NETS)
def test_net_detect_multi_equals_detect_image(model, size, batch, classes):
    n = mnet.Net(prototxt_text=zoo.prototxt(model, batch=batch, **size))
    synth.load_into(n, "mid")
    N, _, H, W = n.blob_shape("data")
    orgs = [(375 + 25 * i, 1242 - 50 * i) for i in range(N)]
    n.set_blob("data", np.concatenate([synth.frame(H, W, seed=31 + 7 * i, org_hw=orgs[i]) for i in range(N)], 0))
    n.forward()
    params = [dict(ratios=(H / float(o[0]), W / float(o[1])), org_hw=o) for o in orgs]
    segs, rois = n.detect_multi(params, classes)
    R = n.blob_shape("proposals_score")[0]
    assert sum(rois) == R and len(segs) == N
    total = 0
    for i in range(N):
        for c, cls_id in enumerate(classes):
            dets, ids, Ri = n.detect_image(i, cls_id, **params[i])
            assert Ri == rois[i]
            assert _same(segs[i][c][0], dets) and np.array_equal(segs[i][c][1], ids), (i, cls_id)
            total += len(dets)
    assert total > 0
    # the device pack: the same result once unpacked
    cap = len(classes) * R
    ptr = n.detect_multi_device(params, classes, cap)
    segs2, rois2 = mnet.unpack_detections_multi(_pack_to_host(ptr, mnet.detect_multi_pack_bytes(N, len(classes), cap)), N, len(classes), cap)
    assert rois2 == rois
    for i in range(N):
        for c in range(len(classes)):
            assert _same(segs2[i][c][0], segs[i][c][0]) and np.array_equal(segs2[i][c][1], segs[i][c][1])
    # errors name the numbers, never truncate
    with pytest.raises(mnet.NetError, match=f"num_images {N + 1} but the net's input holds {N} images"):
        n.detect_multi(params + params[:1], classes)
    if total > 1:
        with pytest.raises(mnet.NetError, match=f"holds {total - 1} rows"):
            n.detect_multi(params, classes, cap=total - 1)
    with pytest.raises(mnet.NetError, match=f"capacity {cap - 1} < {len(classes)} classes x {R} ROIs"):
        n.detect_multi_device(params, classes, cap - 1)


def test_net_detect_multi_batch_one_equals_detect():
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_ped_cyc/mscnn-7s-576-2x", height=192, width=448, max_nms_num=200))
    synth.load_into(n, "mid")
    _, _, H, W = n.blob_shape("data")
    n.set_blob("data", synth.frame(H, W, seed=99))
    n.forward()
    kw = dict(ratios=(H / 375.0, W / 1242.0), org_hw=(375, 1242))
    segs, rois = n.detect_multi([kw], [2, 3])
    for c, cls_id in enumerate((2, 3)):
        dets, ids, R = n.detect(cls_id, **kw)
        assert rois == [R] and _same(segs[0][c][0], dets) and np.array_equal(segs[0][c][1], ids)


def test_net_detect_multi_above_4032_rows_per_image_takes_the_per_segment_path():
    """max_nms_num 5000 (per-image bound over 4032): the per-segment fallback -- tiled kernels, device pack copied -- in the same layout,
    equal to detect_image; a sparse frame next (R_all, hence the bound, under 4032: the one-pass kernels) on the same net."""
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", batch=2, height=192, width=640, max_nms_num=5000, iou_thr=1.01,
                                            min_size=1))
    synth.load_into(n, "dense")
    N, _, H, W = n.blob_shape("data")
    x = np.concatenate([synth.frame(H, W, seed=77 + i) for i in range(N)], 0)
    kw = dict(ratios=(H / 375.0, W / 1242.0), org_hw=(375, 1242))
    for regime, big in (("dense", True), ("sparse", False)):
        synth.set_regime(n, regime)
        n.set_blob("data", x)
        n.forward()
        segs, rois = n.detect_multi([kw] * N, [2, 3])
        assert (max(rois) > 4032) == big, rois
        for i in range(N):
            for c, cls_id in enumerate((2, 3)):
                dets, ids, Ri = n.detect_image(i, cls_id, cap=8192, **kw)
                assert Ri == rois[i] and _same(segs[i][c][0], dets) and np.array_equal(segs[i][c][1], ids), (regime, i, cls_id)
        if big:
            cap = 2 * sum(rois)
            ptr = n.detect_multi_device([kw] * N, [2, 3], cap)
            segs2, _ = mnet.unpack_detections_multi(_pack_to_host(ptr, mnet.detect_multi_pack_bytes(N, 2, cap)), N, 2, cap)
            assert all(_same(segs2[i][c][0], segs[i][c][0]) for i in range(N) for c in range(2))
