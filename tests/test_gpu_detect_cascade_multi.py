"""The one-pass cascade final stage on the GPU: mscnn_detections_cascade_multi_fwd against mscnn_detections_cascade_fwd on every
segment's row range of its output's blobs (bit for bit, ids included) and against the oracle (the assertion of
tests/test_gpu_net.py's cascade check: ids and dets equal), mscnn_net_detect_cascade_multi / _device on batched cascade nets, and
tools/run_cascademscnn.py end to end.  Reduced-size nets only."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from mscnn_amd import net as mnet, synth, zoo   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X: torch.cuda.is_available() is False")
    from mscnn_amd import hipapi
    hipapi.lib()
    return hipapi


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def cascade_outputs(rows_per_image, num_outputs, ncls, seed):
    """[(boxes [R, 5], cls_prob [R, ncls], props [R, 5])] per cascade output, rows grouped by image (column 0 ascending): per image
    clusters of overlapping boxes; every output has boxes, probabilities and proposals of its own (a later stage's proposals are
    the earlier one's boxes, as DecodeBBox chains them); in every output some proposals have x2 = x1 - 1 (zero width, :104-107) or
    y2 = y1 - 1.  ncls: one number, or one per output."""
    rng = np.random.default_rng(seed)
    img = np.concatenate([np.full(n, i, np.float32) for i, n in enumerate(rows_per_image)]) if len(rows_per_image) else np.zeros(0, np.float32)
    R = len(img)
    parts = []
    for n in rows_per_image:
        c = rng.uniform(0, 1000, (max(1, n // 8), 2))
        xy = c[rng.integers(0, len(c), n)] + rng.normal(0, 10, (n, 2))
        wh = rng.uniform(40, 160, (n, 2))
        parts.append(np.concatenate([xy, xy + wh], 1))
    base = np.concatenate(parts, 0).astype(np.float32) if R else np.zeros((0, 4), np.float32)
    outs, prev = [], base
    for o in range(num_outputs):
        props = np.concatenate([img[:, None], prev], 1).astype(np.float32)
        boxes = np.concatenate([img[:, None], prev + rng.normal(0, 6, (R, 4)).astype(np.float32)], 1).astype(np.float32)
        logits = rng.standard_normal((R, ncls[o] if isinstance(ncls, (list, tuple)) else ncls)) * 1.5
        prob = (np.exp(logits) / np.exp(logits).sum(1, keepdims=True)).astype(np.float32)
        prob[3::11] = prob[2::11][: len(prob[3::11])]                    # exact ties: the sort is stable
        props[4 + o::13, 3] = props[4 + o::13, 1] - 1                    # zero width
        props[9 + o::31, 4] = props[9 + o::31, 2] - 1                    # zero height
        outs.append((boxes, prob, props))
        prev = boxes[:, 1:]
    return outs


def image_kw(i):
    org = (375 + 40 * i, 1242 - 60 * i)
    return dict(ratios=(576 / org[0], 1920 / org[1]), org_hw=org, nms_overlap=0.5 if i % 2 == 0 else 0.4)


def ranges_of(props, num_images):
    img = props[:, 0].astype(int)
    return [(int(np.searchsorted(img, i, "left")), int(np.searchsorted(img, i, "right") - np.searchsorted(img, i, "left"))) for i in range(num_images)]


def survivors(prob, props, cls_id, det_thr):
    p = prob[:, cls_id - 1]
    ok = (props[:, 3] - props[:, 1] + np.float32(1) != 0) & (props[:, 4] - props[:, 2] + np.float32(1) != 0) & ~np.isnan(p)
    return ok & (p >= np.float32(det_thr)) if det_thr > 0 else ok


def oracle_segments(orc, outs, num_images, classes, det_thr, kw_of=image_kw, seg_kw=lambda i, o, c: {}):
    """[(dets, ids, row0, rows, survivors)] per segment, image-major, then output, then class, from the CPU oracle.  seg_kw(image,
    output, cls_id): keyword arguments of that one segment, over kw_of(image)'s."""
    res = []
    for i in range(num_images):
        for o, (boxes, prob, props) in enumerate(outs):
            row0, rows = ranges_of(props, num_images)[i]
            sl = slice(row0, row0 + rows)
            for c in classes:
                d, ids = orc.detections_cascade(boxes[sl], prob[sl], props[sl], cls_id=c, det_thr=det_thr, **dict(kw_of(i), **seg_kw(i, o, c)))
                res.append((d, ids, row0, rows, int(survivors(prob[sl], props[sl], c, det_thr).sum())))
    return res


def check_op(hip, outs, num_images, classes, det_thr, want, max_rows=None, kw_of=image_kw, seg_kw=lambda i, o, c: {}):
    """The one-pass op against the per-range op (bit for bit) and against the oracle's segments `want` (ids and dets equal: the
    assertion of test_gpu_net._check_cascade)."""
    segs = [dict(kw_of(i), cls_id=c, **seg_kw(i, o, c)) for i in range(num_images) for o in range(len(outs)) for c in classes]
    douts = [tuple(dev(t) for t in o) for o in outs]
    got = hip.detections_cascade_multi(douts, num_images, segs, det_thr=det_thr, max_rows_per_image=max_rows)
    assert len(got) == len(want) == len(segs)
    K = len(outs) * len(classes)
    for s, (dets, ids, row0, rows) in enumerate(got):
        o = (s % K) // len(classes)
        dref, iref, want0, wantn, _ = want[s]
        assert (row0, rows) == (want0, wantn), (s, row0, rows)
        sl = slice(row0, row0 + rows)
        boxes, prob, props = outs[o]
        d1, i1 = hip.detections_cascade(dev(boxes[sl]), dev(prob[sl]), dev(props[sl]), det_thr=det_thr, **segs[s])
        assert np.array_equal(ids, i1.cpu().numpy()), s                      # the per-call stage on the range: bit for bit
        assert _same(dets, d1.cpu().numpy()), s
        assert np.array_equal(ids, iref) and np.array_equal(dets, dref), s   # the oracle: selection, order and values
    return got


OP_CASES = [   # rows per image, cascade outputs, classes, det_thr
    ([150], 1, [2], 0.0),
    ([90], 3, [2, 3], 0.0),
    ([40, 120, 64], 1, [2, 3], 0.25),
    ([65, 24, 200], 3, [2], 0.0),
    ([70, 33, 128, 21], 3, [2, 3, 4], 0.2),          # 36 segments: two chunks of launches
]


@pytest.mark.parametrize("rows,O,classes,det_thr", OP_CASES)
def test_cascade_multi_op_every_segment_equals_the_per_range_stage(hip, orc, rows, O, classes, det_thr):
    outs = cascade_outputs(rows, O, 4, 100 + len(rows) + 10 * O + len(classes))
    B = len(rows)
    want = oracle_segments(orc, outs, B, classes, det_thr)
    # the inputs do not let the test pass vacuously -- asserted on the oracle's output, before the device is looked at
    assert min(rows) >= 20
    assert any(0 < len(d) < surv for d, _, _, _, surv in want)                                   # the NMS suppresses
    for boxes, prob, props in outs:
        assert ((props[:, 3] - props[:, 1] + 1 == 0) | (props[:, 4] - props[:, 2] + 1 == 0)).any()   # the zero-size filter drops rows
    if det_thr > 0:
        p = np.concatenate([prob[:, c - 1] for _, prob, _ in outs for c in classes])
        assert (p < det_thr).any() and (p >= det_thr).any()
        assert any(surv < r for _, _, _, r, surv in want) and any(surv > 0 for *_, surv in want)
    if O > 1:
        for a in range(O):
            for b in range(a + 1, O):
                assert not np.array_equal(outs[a][0], outs[b][0]) and not np.array_equal(outs[a][1], outs[b][1])
        assert len({tuple(ids.tolist()) for d, ids, *_ in want[:O * len(classes):len(classes)]}) == O      # and so do their results
    if B * O * len(classes) > 32:
        assert B * O * len(classes) == 36
    check_op(hip, outs, B, classes, det_thr, want, max_rows=max(rows))
    if O == 3 and len(classes) == 1:                 # the loosest host bound: every row of the batch
        check_op(hip, outs, B, classes, det_thr, want)


def test_cascade_multi_op_chunk_boundary_inside_an_image_and_outputs_of_different_width(hip, orc):
    """2 images x 3 outputs x 6 classes = 36 segments: the second chunk of launches starts at segment 32 = (image 1, output 2, third
    class), inside an image and between two classes of one output, so the chunk-local segment index differs from the global one.  The
    outputs have 7, 7 and 8 probability columns (the segment's source decides the row stride); the images have 65 rows (one past a
    64-bit mask word) and 1 row; one segment of each image has an nms_overlap of its own."""
    rows, classes, ncls = [65, 1], [2, 3, 4, 5, 6, 7], (7, 7, 8)
    outs = cascade_outputs(rows, 3, ncls, 301)
    assert [o[1].shape[1] for o in outs] == list(ncls)
    own = lambda i, o, c: dict(nms_overlap=0.2) if (o, c) == (1, 4) else {}      # noqa: E731
    want = oracle_segments(orc, outs, 2, classes, 0.0, seg_kw=own)
    assert len(want) == 36 and 32 // 18 == 1 and (32 % 18) // 6 == 2 and 32 % 6 == 2
    # not vacuous, on the oracle's output: the NMS suppresses in every segment of image 0, the single row of image 1 is a detection
    # everywhere, and the segment with its own overlap differs from what its image's overlap gives
    assert all(0 < len(d) < surv for d, _, _, _, surv in want[:18])
    assert all(len(d) == 1 and (row0, n) == (65, 1) for d, _, row0, n, _ in want[18:])
    plain = oracle_segments(orc, outs, 2, classes, 0.0)
    assert len(want[6 + 2][0]) < len(plain[6 + 2][0])
    assert all(np.array_equal(a[0], b[0]) for s, (a, b) in enumerate(zip(want, plain)) if s % 18 != 8)
    check_op(hip, outs, 2, classes, 0.0, want, max_rows=65, seg_kw=own)


def test_cascade_multi_op_edge_rows(hip, orc):
    """An image without rows between two that have some; the whole-batch dummy row of an empty BoxOutput; NaN probabilities; an image
    over max_rows_per_image."""
    outs = cascade_outputs([25, 0, 30], 2, 3, 7)
    want = oracle_segments(orc, outs, 3, [2, 3], 0.0)
    got = check_op(hip, outs, 3, [2, 3], 0.0, want, max_rows=30)
    assert [(len(g[0]), g[3]) for g in got[4:8]] == [(0, 0)] * 4 and all(g[2] == 25 for g in got[4:8])
    assert all(len(g[0]) > 0 for g in got[:4] + got[8:])
    # the neighbours are what they are without the empty image in between
    alone = cascade_outputs([25, 0, 30], 2, 3, 7)
    for t in alone:
        t[0][25:, 0] = 1; t[2][25:, 0] = 1
    kw_skip = lambda i: image_kw(2 * i)              # noqa: E731  (images 0 and 2 of the batch above)
    got2 = check_op(hip, alone, 2, [2, 3], 0.0, oracle_segments(orc, alone, 2, [2, 3], 0.0, kw_skip), max_rows=30, kw_of=kw_skip)
    for a, b in zip(got[:4] + got[8:], got2):
        assert _same(a[0], b[0]) and np.array_equal(a[1], b[1])
    # [0 1 1 10 10]: the row an empty BoxOutput emits for the whole batch lands in image 0
    z = np.array([[0, 1, 1, 10, 10]], np.float32)
    dummy = [(z.copy(), np.array([[0.25, 0.75]], np.float32), z.copy())]
    want = oracle_segments(orc, dummy, 3, [2], 0.0)
    got = check_op(hip, dummy, 3, [2], 0.0, want)
    assert [(g[2], g[3]) for g in got] == [(0, 1), (1, 0), (1, 0)] and [len(g[0]) for g in got] == [1, 0, 0]
    # NaN probabilities drop out (bbNms.m:76)
    outs = cascade_outputs([40, 40], 1, 3, 9)
    outs[0][1][5::6, 1] = np.nan
    want = oracle_segments(orc, outs, 2, [2], 0.0)
    assert all(len(d) > 0 and not np.isnan(d).any() and not ((ids + row0) % 6 == 5).any() for d, ids, row0, *_ in want)
    check_op(hip, outs, 2, [2], 0.0, want, max_rows=40)
    # an image over the bound: count -1 for its segments, the others run; the unpacker names the image
    outs = cascade_outputs([20, 50, 20], 2, 3, 11)
    segs = [dict(cls_id=2, **image_kw(i)) for i in range(3) for _ in outs]
    got = hip.detections_cascade_multi([tuple(dev(t) for t in o) for o in outs], 3, segs, max_rows_per_image=40)
    want = oracle_segments(orc, outs, 3, [2], 0.0)
    for s, g in enumerate(got):
        if s // 2 == 1:
            assert g[0] is None and (g[2], g[3]) == (20, 50)
        else:
            assert np.array_equal(g[1], want[s][1]) and np.array_equal(g[0], want[s][0])


def test_cascade_multi_keeps_images_apart(hip, orc):
    """Two images with IDENTICAL boxes and probabilities: the one-pass stage returns the same detections for both, each equal to the
    single-image result.  (mscnn_detections_cascade_fwd / Net.detect_cascade on the same two-image blob treat it as one list: every
    box of image 1 has an identical, earlier box of image 0, so it returns the detections of ONE image -- fewer than the two images
    have; that behaviour is not asserted here.)"""
    one = cascade_outputs([80], 2, 3, 21)
    two = []
    for boxes, prob, props in one:
        b2, q2 = boxes.copy(), props.copy()
        b2[:, 0] = 1; q2[:, 0] = 1
        two.append((np.concatenate([boxes, b2]), np.concatenate([prob, prob]), np.concatenate([props, q2])))
    kw = lambda i: image_kw(0)                       # noqa: E731
    w1 = oracle_segments(orc, one, 1, [2, 3], 0.0, kw)
    assert all(0 < len(d) for d, *_ in w1) and any(len(d) < surv for d, _, _, _, surv in w1)
    g1 = check_op(hip, one, 1, [2, 3], 0.0, w1, kw_of=kw)
    g2 = check_op(hip, two, 2, [2, 3], 0.0, oracle_segments(orc, two, 2, [2, 3], 0.0, kw), max_rows=80, kw_of=kw)
    for k in range(4):
        for img in range(2):
            assert _same(g2[4 * img + k][0], g1[k][0]) and np.array_equal(g2[4 * img + k][1], g1[k][1])


# ---- the net entries ---------------------------------------------------------------------------------------------------------------
def frame_u8(h, w, seed):
    """uint8 RGB [h, w, 3] frame of the seeded generator (synth.frame at its own size, mean added back)."""
    x = synth.frame(h, w, seed=seed, org_hw=(h, w))[0].transpose(1, 2, 0)[:, :, ::-1] + np.array([123.0, 117.0, 104.0])
    return np.ascontiguousarray(np.clip(np.round(x), 0, 255).astype(np.uint8))


def outputs_of(n):
    return [("output_bbox_1st", "cls_prob_1st", "proposals"), ("output_bbox_2nd", "cls_prob_2nd", "proposals_2nd"),
            ("output_bbox_3rd", "cls_prob_3rd_avg" if "cls_prob_3rd_avg" in n.blob_names else "cls_prob_3rd", "proposals_3rd")]


def _pack_to_host(ptr, nbytes):
    torch.cuda.synchronize()
    hiprt = C.CDLL("libamdhip64.so")
    host = np.zeros(nbytes, np.uint8)
    assert hiprt.hipDeviceSynchronize() == 0
    assert hiprt.hipMemcpy(host.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(nbytes), 2) == 0      # hipMemcpyDeviceToHost
    return host


def check_net_segments(hip, orc, n, per_image, rois, params, outputs, classes, det_thr=0.0):
    """Every (i, o, c) of a detect_cascade_multi result against the per-range op and the oracle on the blobs read back from the net
    (the final stage on whatever the forward produced)."""
    B = len(params)
    total = 0
    for o, (bb, pb, qb) in enumerate(outputs):
        R = n.blob_shape(bb)[0]
        boxes, prob, props = n.get_blob(bb).reshape(R, 5), n.get_blob(pb).reshape(R, -1), n.get_blob(qb).reshape(R, 5)
        rng = ranges_of(props, B)
        assert [r[1] for r in rng] == rois and sum(rois) == R
        for i, (row0, rows) in enumerate(rng):
            sl = slice(row0, row0 + rows)
            for c, cls_id in enumerate(classes):
                kw = dict(cls_id=cls_id, det_thr=det_thr, ratios=params[i]["ratios"], org_hw=params[i]["org_hw"])
                dets, ids = per_image[i][o][c]
                d1, i1 = hip.detections_cascade(dev(boxes[sl]), dev(prob[sl]), dev(props[sl]), **kw)
                assert _same(dets, d1.cpu().numpy()) and np.array_equal(ids - row0, i1.cpu().numpy()), (i, o, cls_id)
                dref, iref = orc.detections_cascade(boxes[sl], prob[sl], props[sl], **kw)
                assert np.array_equal(ids - row0, iref) and np.array_equal(dets, dref), (i, o, cls_id)
                total += len(dets)
    return total


@pytest.mark.parametrize("model,size,classes", [
    ("kitti_car/cascade-mscnn-7s-576-2x", dict(height=192, width=448, max_nms_num=150), [2, 3]),
    ("widerface/cascade-mscnn-12s-align", dict(height=160, width=192, max_nms_num=150), [2]),
])
def test_net_detect_cascade_multi_on_batched_cascade_nets(hip, orc, model, size, classes):
    """batch 2, two different frames of different sizes through set_images, forward, one detect_cascade_multi over the three cascade
    outputs: every (image, output, class) equals the per-range op (bit for bit) and the oracle on rows [row0_i, + rows_i) of the
    blobs read back.  No claim about the batched cascade forward itself."""
    n = mnet.Net(prototxt_text=zoo.prototxt(model, batch=2, **size))
    synth.load_into(n, "mid")
    params = n.set_images("data", [frame_u8(375, 1242, 41), frame_u8(300, 900, 42)])
    n.forward()
    outputs = outputs_of(n)
    per_image, rois = n.detect_cascade_multi(params, outputs, classes)
    assert len(per_image) == 2 and min(rois) > 3, rois
    total = check_net_segments(hip, orc, n, per_image, rois, params, outputs, classes)
    assert total > 0
    # the device pack: the same result once unpacked
    R = sum(rois)
    cap = 3 * len(classes) * R
    ptr = n.detect_cascade_multi_device(params, outputs, classes, cap)
    host = _pack_to_host(ptr, mnet.detect_cascade_multi_pack_bytes(2, 3, len(classes), cap))
    per2, rois2 = mnet.unpack_detections_cascade_multi(host, 2, 3, len(classes), cap)
    assert rois2 == rois
    for i in range(2):
        for o in range(3):
            for c in range(len(classes)):
                assert _same(per2[i][o][c][0], per_image[i][o][c][0]) and np.array_equal(per2[i][o][c][1], per_image[i][o][c][1])
    # errors name the numbers, never truncate
    with pytest.raises(mnet.NetError, match="num_images 3 but the net's input holds 2 images"):
        n.detect_cascade_multi(params + params[:1], outputs, classes)
    with pytest.raises(mnet.NetError, match=f"holds {total - 1} rows"):
        n.detect_cascade_multi(params, outputs, classes, cap=total - 1)
    with pytest.raises(mnet.NetError, match=f"capacity {cap - 1} < 3 outputs x {len(classes)} classes x {R} ROIs"):
        n.detect_cascade_multi_device(params, outputs, classes, cap - 1)


def test_net_detect_cascade_multi_batch_one_equals_detect_cascade():
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/cascade-mscnn-7s-576-2x", height=192, width=448, max_nms_num=150))
    synth.load_into(n, "mid")
    params = n.set_images("data", [frame_u8(375, 1242, 43)])
    n.forward()
    for bb, pb, qb in outputs_of(n):
        for det_thr in (0.0, 0.1):
            per_image, rois = n.detect_cascade_multi(params, [(bb, pb, qb)], [2], det_thr=det_thr)
            dets, ids, R = n.detect_cascade(bb, pb, qb, cls_id=2, det_thr=det_thr, **params[0])
            assert rois == [R] and R > 3
            assert _same(per_image[0][0][0][0], dets) and np.array_equal(per_image[0][0][0][1], ids), (bb, det_thr)


def test_net_detect_cascade_multi_above_4032_rows_per_image_takes_the_per_segment_path(hip, orc):
    """max_nms_num 5000 on a dense frame pair (the settings of test_gpu_detect_multi's fallback test): more than 4032 rows per image,
    so the per-segment fallback -- tiled kernels, device pack copied -- fills the same layout; compared with the per-range op and the
    oracle like the one-pass path.  One output and one class keep it short."""
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/cascade-mscnn-7s-576-2x", batch=2, height=192, width=640, max_nms_num=5000,
                                            iou_thr=1.01, min_size=1))
    synth.load_into(n, "dense")
    params = n.set_images("data", [frame_u8(375, 1242, 44), frame_u8(320, 1000, 45)])
    n.forward()
    outputs = outputs_of(n)[2:]
    per_image, rois = n.detect_cascade_multi(params, outputs, [2], det_thr=0.05)
    assert max(rois) > 4032, rois
    assert check_net_segments(hip, orc, n, per_image, rois, params, outputs, [2], det_thr=0.05) > 0
    cap = sum(rois)
    ptr = n.detect_cascade_multi_device(params, outputs, [2], cap, det_thr=0.05)
    per2, _ = mnet.unpack_detections_cascade_multi(_pack_to_host(ptr, mnet.detect_cascade_multi_pack_bytes(2, 1, 1, cap)), 2, 1, 1, cap)
    assert all(_same(per2[i][0][0][0], per_image[i][0][0][0]) for i in range(2))


# ---- the driver --------------------------------------------------------------------------------------------------------------------
def _run_driver(tmp_path, tag, *args):
    out = tmp_path / tag
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools/run_cascademscnn.py"), "--out", str(out), "--comp-id", "t", *args],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return {f: (out / f).read_bytes() for f in sorted(os.listdir(out))}


def test_driver_batch_two_and_batch_one_write_the_per_range_stage_of_their_own_blobs(hip, tmp_path):
    """tools/run_cascademscnn.py on the reduced kitti_car cascade, four synthetic frames of two sizes, outputs 1st,2nd,3rd, with
    --batch 2 and with --batch 1: the same set of result files.  Their bytes are NOT compared with each other: the forward's blobs
    differ in the last bits between batch sizes (measured on the MI355X: one probability of the 2nd output printed as 0.021725 at
    batch 2 and 0.021724 at batch 1, everything else equal -- the GEMM layers' summation order depends on the row count), which is
    the forward's business, not this stage's.  Instead each run's files must be, byte for byte, what the per-range op
    (mscnn_detections_cascade_fwd on each image's rows) gives on that run's OWN blobs (--dump-blobs)."""
    from mscnn_amd import kitti
    common = ["--model", "kitti_car/cascade-mscnn-7s-576-2x", "--input-size", "192,448", "--max-nms-num", "150", "--synthetic", "4",
              "--synthetic-sizes", "375x1242,300x900", "--outputs", "1st,2nd,3rd"]
    names = ["t_car_1st_results.txt", "t_car_2nd_results.txt", "t_car_3rd_results.txt"]
    triples = [("output_bbox_1st", "cls_prob_1st", "proposals"), ("output_bbox_2nd", "cls_prob_2nd", "proposals_2nd"),
               ("output_bbox_3rd", "cls_prob_3rd", "proposals_3rd")]
    for batch in (2, 1):
        dump = tmp_path / f"blobs{batch}"
        files = _run_driver(tmp_path, f"b{batch}", *common, "--batch", str(batch), "--dump-blobs", str(dump))
        assert sorted(files) == names and all(len(v) > 0 for v in files.values())
        groups = sorted(os.listdir(dump))
        assert len(groups) == 4 // batch
        per_output = [[] for _ in triples]
        for g in groups:
            z = np.load(dump / g)
            for i in range(batch):
                for o, (bb, pb, qb) in enumerate(triples):
                    R = z[bb].shape[0]
                    boxes, prob, props = z[bb].reshape(R, 5), z[pb].reshape(R, -1), z[qb].reshape(R, 5)
                    row0, rows = ranges_of(props, batch)[i]
                    sl = slice(row0, row0 + rows)
                    d, _ = hip.detections_cascade(dev(boxes[sl]), dev(prob[sl]), dev(props[sl]), cls_id=2, det_thr=0.0,
                                                  ratios=tuple(z["ratios"][i]), org_hw=tuple(z["org_hw"][i]))
                    per_output[o].append(d.cpu().numpy())
        for o, name in enumerate(names):
            want = tmp_path / f"want{batch}_{name}"
            kitti.write_detections_dlm(str(want), per_output[o])
            assert files[name] == want.read_bytes(), (batch, name)


def test_driver_orig_size_reshapes_between_frames(tmp_path):
    """--orig-size over two synthetic frames of different sizes on the reduced WiderFace deploy: Net.reshape_input between frames."""
    files = _run_driver(tmp_path, "wf", "--model", "widerface/cascade-mscnn-12s-align", "--input-size", "160,192", "--max-nms-num", "150",
                        "--synthetic", "2", "--synthetic-sizes", "150x200,200x170", "--orig-size", "--names", "bg,face", "--det-thr", "0.05")
    assert list(files) == ["t_face_3rd_avg_results.txt"]
