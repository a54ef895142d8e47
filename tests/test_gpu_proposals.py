"""The proposal half of the scripts' result on the GPU: mscnn_proposals_multi_fwd against the numpy witness of
run_mscnn_detection.m:75-91 (tests/proposals_witness.py) bit for bit -- doubles as uint64, rows, counts and the {count, rows, row0}
table exactly --, and mscnn_net_proposals_multi / _device / mscnn_net_forward_proposals on reduced deploys.  All data is synthetic
and seeded.  The stage has no pin on the reference (no MATLAB): the witness is its check."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from mscnn_amd import net as mnet, synth, zoo   # noqa: E402
from proposals_witness import RATIOS, batch_witness, synth_props   # noqa: E402


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X: torch.cuda.is_available() is False")
    from mscnn_amd import hipapi
    hipapi.lib()
    return hipapi


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def images_for(n):
    return [dict(ratios=RATIOS[i % len(RATIOS)]) for i in range(n)]


def check_op(hip, props, images):
    """The op on props against the witness: every image's rows, order, bits; the pack's header and table word for word."""
    out, raw = hip.proposals_multi(dev(props), images, raw_pack=True)
    want = batch_witness(props, images)
    B, R = len(images), len(props)
    table = raw[:16 * (B + 1)].view(np.int32).reshape(B + 1, 4)
    assert table[0].tolist() == [B, R, R, 0]
    assert table[1:].tolist() == [[len(p), rows, row0, 0] for p, _, row0, rows in want]
    kept = 0
    for i, ((p, rows, row0, n), (wp, wk, wrow0, wn)) in enumerate(zip(out, want)):
        assert (row0, n) == (wrow0, wn), i
        assert p.shape == wp.shape and np.array_equal(bits(p), bits(wp)), i
        assert rows.dtype == np.int32 and np.array_equal(rows, wk), i
        kept += len(p)
    return want, kept


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 1025])
def test_one_image_rows_around_the_wave_and_step_sizes(hip, n):
    """64 rows per ballot, 256 per step: one under, on and over each; about half of the rows filtered."""
    props = synth_props([n], 100 + n)
    _, kept = check_op(hip, props, images_for(1))
    if n >= 63:
        assert 0.3 * n < kept < 0.7 * n, (n, kept)


@pytest.mark.parametrize("rows,seed", [([65, 0, 1, 130], 11), ([0, 0, 5], 13)])
def test_batches_with_empty_images(hip, rows, seed):
    """An empty image between others, and an empty FIRST image (seeds chosen on the witness: every non-empty image keeps a row)."""
    want, _ = check_op(hip, synth_props(rows, seed), images_for(len(rows)))
    assert [w[3] for w in want] == rows and all(len(w[0]) > 0 for w in want if w[3])


def test_one_more_image_than_a_launch_group(hip):
    B = hip.PROPOSALS_IMAGES_PER_LAUNCH + 1
    rows = [(5 * i + 3) % 4 for i in range(B)]      # 0 - 3 rows each
    assert set(rows) == {0, 1, 2, 3} and rows[-1] > 0
    props = synth_props(rows, 19)
    props[:, 5] = np.where(np.arange(len(props)) % 3 == 0, -11.0, props[:, 5] + 20.0)      # a third filtered, whatever the seed
    want, kept = check_op(hip, props, images_for(B))
    assert kept > 0 and len(want[-1][0]) > 0      # the image of the second launch has rows of its own


def test_whole_batch_dummy_row(hip):
    """The [0 0 0 0 0 0] row BoxOutput emits when nothing survives in the whole batch: image 0 owns it and filters it (w == 0)."""
    out, raw = hip.proposals_multi(dev(np.zeros((1, 6), np.float32)), images_for(3), raw_pack=True)
    assert raw[:64].view(np.int32).reshape(4, 4).tolist() == [[3, 1, 1, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 1, 0]]
    assert [len(o[0]) for o in out] == [0, 0, 0]
    check_op(hip, np.zeros((1, 6), np.float32), images_for(3))


def test_edge_rows(hip):
    nan, inf = float("nan"), float("inf")
    props = np.array([
        [0, 10, 20, 110, 70, -10.0],                # score == proposal_thr: kept
        [0, 10, 20, 110, 70, -10.000001],           # one float under it
        [0, 10, 20, 110, 70, nan],
        [0, 10, 20, 110, 70, inf],                  # kept
        [0, 10, 20, 110, 70, -inf],
        [0, 30, 20, 30, 70, 2.0],                   # x2 == x1 with h != 0
        [0, 30, 20, 40, 20, 2.0],                   # y2 == y1
        [0, -0.0, 20, 0.0, 70, 2.0],                # +0 extent
        [0, 0.0, 20, -0.0, 70, 2.0],                # -0 extent: zero too
        [0, 50, 20, 40, 70, 3.0],                   # negative width: kept
        [0, 0.1, 0.2, 0.4, 0.7, 0.0],               # fp32 extents
        [1, 10, 20, 110, 70, -3.0],                 # image 1 with its own threshold: -3 >= -3 kept
        [1, 10, 20, 110, 70, -3.0000002],           # dropped there, although >= -10
    ], np.float32)
    images = [dict(ratios=RATIOS[0]), dict(ratios=RATIOS[1], proposal_thr=-3.0)]
    want, _ = check_op(hip, props, images)
    assert want[0][1].tolist() == [0, 3, 9, 10] and want[1][1].tolist() == [0]
    assert want[0][0][2, 2] < 0 and want[0][0][1, 4] == inf


def test_more_rows_than_the_final_stage_holds_in_one_list(hip):
    """4100 rows in one image (> 4032): the same code, nothing to sort, no bit matrix."""
    want, kept = check_op(hip, synth_props([4100, 37], 3), images_for(2))
    assert len(want[0][0]) > 1500 and len(want[1][0]) > 5


def test_ratios_per_image_and_the_division_is_the_double_one(hip):
    """576/375 and 1920/1242 in image 0, other ratios in the others; the data tells the float64 division from the fp32 one."""
    props = synth_props([200, 90, 33], 42)
    images = images_for(3)
    assert images[0]["ratios"] == (576 / 375.0, 1920 / 1242.0) and len({im["ratios"] for im in images}) == 3
    want, _ = check_op(hip, props, images)
    alt = batch_witness(props, images, f32_division=True)
    for (p, k, _, _), (q, kq, _, _) in zip(want, alt):
        assert np.array_equal(k, kq) and not np.array_equal(bits(p[:, :4]), bits(q[:, :4]))


def test_rows_past_each_count_and_bytes_past_the_pack_stay(hip):
    props = synth_props([70, 0, 300, 5], 8)
    images = images_for(4)
    B, R = 4, len(props)
    nbytes = hip.lib().mscnn_proposals_multi_pack_bytes(B, R)
    pack = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    _, raw = hip.proposals_multi(dev(props), images, raw_pack=True, pack=pack)
    want = batch_witness(props, images)
    exp = np.full(nbytes + 256, 0xA5, np.uint8)
    table = 16 * (B + 1)
    exp[:table].view(np.int32).reshape(B + 1, 4)[:] = [[B, R, R, 0]] + [[len(p), rows, row0, 0] for p, _, row0, rows in want]
    dets = exp[table:table + 40 * R].view(np.float64).reshape(-1, 5)
    ids = exp[table + 40 * R:table + 44 * R].view(np.int32)
    for p, k, row0, rows in want:
        assert 0 < len(p) < rows or rows == 0
        dets[row0:row0 + len(p)] = p
        ids[row0:row0 + len(p)] = k
    assert np.array_equal(raw, exp)


# ---- the net entries ---------------------------------------------------------------------------------------------------------------
NETS = [   # model, reduced input, batch, classes, frame sizes
    ("kitti_ped_cyc/mscnn-7s-576-2x", dict(height=192, width=448, max_nms_num=200), 1, [2, 3], [(375, 1242)]),
    ("kitti_car/mscnn-7s-576", dict(height=192, width=640, max_nms_num=200), 3, [2], [(375, 1242), (370, 1224), (300, 900)]),
]


def _pack_to_host(ptr, nbytes):
    torch.cuda.synchronize()
    hiprt = C.CDLL("libamdhip64.so")
    host = np.zeros(nbytes, np.uint8)
    assert hiprt.hipDeviceSynchronize() == 0
    assert hiprt.hipMemcpy(host.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(nbytes), 2) == 0      # hipMemcpyDeviceToHost
    return host


def _same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def _frames(sizes):
    return [np.random.default_rng(900 + i).integers(0, 256, (h, w, 3), dtype=np.uint8) for i, (h, w) in enumerate(sizes)]


@pytest.mark.parametrize("model,size,batch,classes,sizes", NETS)
def test_net_proposals_and_the_rpn_only_run(model, size, batch, classes, sizes):
    text = zoo.prototxt(model, batch=batch, **size)
    fresh, n = mnet.Net(prototxt_text=text), mnet.Net(prototxt_text=text)
    shapes = [n.param_shapes(i) for i in range(len(n.layer_names))]
    ws = synth.weights(n.layer_names, n.layer_types, shapes, "mid")
    for net in (fresh, n):
        for name, blobs in ws.items():
            for p, arr in enumerate(blobs):
                net.set_param(name, p, arr)
    frames = _frames(sizes)
    # the fresh net: a whole forward, its final stage, its proposals
    params = fresh.set_images("data", frames)
    fresh.forward()
    ps = fresh.get_blob("proposals_score").reshape(-1, 6)
    R = len(ps)
    ref_blobs = {b: fresh.get_blob(b) for b in ("bbox_pred", "cls_pred")}
    segs, rois = fresh.detect_multi(params, classes)
    got, rois_p = fresh.proposals_multi(params)
    want = batch_witness(ps, params)
    assert rois_p == rois == [w[3] for w in want] and sum(rois) == R
    assert sum(len(w[0]) for w in want) > 0
    for i, ((p, rows), (wp, wk, row0, _)) in enumerate(zip(got, want)):
        assert _same(p, wp) and rows.dtype == np.int32 and np.array_equal(rows, wk + row0), i      # rows of the net's ROI blobs
        for c in range(len(classes)):                                                             # proposals(bbs_show(:,6),:): a join
            assert np.isin(segs[i][c][1], rows).all(), (i, c)
    assert sum(len(s[1]) for row in segs for s in row) > 0
    # the device pack read back: the blocking call
    ptr = fresh.proposals_multi_device(params, R)
    got2, rois2 = mnet.unpack_detections_multi(_pack_to_host(ptr, mnet.detect_multi_pack_bytes(batch, 1, R)), batch, 1, R)
    assert rois2 == rois and all(_same(a[0][0], b[0]) and np.array_equal(a[0][1], b[1]) for a, b in zip(got2, got))
    # errors name the numbers
    with pytest.raises(mnet.NetError, match=f"num_images {batch + 1} but the net's input holds {batch} images"):
        fresh.proposals_multi(params + params[:1])
    with pytest.raises(mnet.NetError, match=f"capacity {R - 1} < {R} ROIs"):
        fresh.proposals_multi_device(params, R - 1)
    total = sum(len(p) for p, _ in got)
    assert total > 1
    with pytest.raises(mnet.NetError, match=f"holds {total - 1} rows"):
        fresh.proposals_multi(params, cap=total - 1)
    # the RPN-only run after a whole forward: the same proposals_score, BoxOutput's index
    last = fresh.forward_proposals()
    assert fresh.layer_types[last] == "BoxOutput" and fresh.layer_tops(last)[1] == "proposals_score"
    assert np.array_equal(fresh.get_blob("proposals_score").reshape(-1, 6).view(np.uint32), ps.view(np.uint32))
    # ... and as the FIRST call on a net: the same blob and proposals, then a whole forward + final stage equal to the fresh net's
    n.set_numerics_watch(1)      # (every whole forward is a watch frame: the RPN-only run must not be counted as one)
    assert n.set_images("data", frames) == params
    assert n.forward_proposals() == last
    assert n.numerics_watch_state()[0] == 0
    assert np.array_equal(n.get_blob("proposals_score").reshape(-1, 6).view(np.uint32), ps.view(np.uint32))
    got3, _ = n.proposals_multi(params)
    assert all(_same(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(got3, got))
    n.set_numerics_watch(25)
    n.forward()
    for b, ref in ref_blobs.items():
        assert np.array_equal(n.get_blob(b).view(np.uint32), ref.view(np.uint32)), b
    segs3, rois3 = n.detect_multi(params, classes)
    assert rois3 == rois
    for i in range(batch):
        for c in range(len(classes)):
            assert _same(segs3[i][c][0], segs[i][c][0]) and np.array_equal(segs3[i][c][1], segs[i][c][1]), (i, c)


def test_a_cascade_deploy_is_refused_by_name():
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/cascade-mscnn-7s-576-2x", height=192, width=448, max_nms_num=200))
    kw = dict(ratios=(192 / 375.0, 448 / 1242.0))
    with pytest.raises(mnet.NetError, match="cascade deploy .DecodeBBox layer proposals_2nd.*proposals_score"):
        n.proposals_multi([kw])
    with pytest.raises(mnet.NetError, match="cascade deploy .DecodeBBox layer proposals_2nd.*proposals_score"):
        n.proposals_multi_device([kw], 200)
