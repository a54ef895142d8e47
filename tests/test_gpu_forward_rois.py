"""The detection sub-net on caller-supplied ROIs on the GPU: mscnn_rois_ingest_f32 against an exact numpy restatement of the
formulas in include/mscnn_hip.h, mscnn_net_forward_rois bit for bit against forward() on the rows BoxOutput itself selected (reduced
deploys: plain, "-2x", cascade, the ROIAlign cascade with its one-pass head off and on), arbitrary boxes against the reference's CPU
layers, what the call leaves behind, and the driver's --rois-in.  All data is synthetic and seeded."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from mscnn_amd import net as mnet, synth, zoo   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS = [(576 / 375.0, 1920 / 1242.0), (0.7, 1.3), (1.0, 1.0)]      # (ratio_h, ratio_w): no fp32 numbers among the first two


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X: torch.cuda.is_available() is False")
    from mscnn_amd import hipapi
    hipapi.lib()
    return hipapi


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the op --------------------------------------------------------------------------------------------------------------------------
def synth_rows(counts, seed, image_form):
    """Rows grouped by image: fp32 [img x1 y1 x2 y2 score] or float64 [img x y w h score] with fractional coordinates, some boxes
    reaching outside a 1242 x 375 frame, some of zero or negative extent."""
    rng = np.random.default_rng(seed)
    R = int(sum(counts))
    rows = np.zeros((R, 6), np.float64)
    rows[:, 0] = np.repeat(np.arange(len(counts)), counts)
    rows[:, 1] = rng.uniform(-50, 1300, R)
    rows[:, 2] = rng.uniform(-30, 400, R)
    rows[:, 3] = rng.uniform(-5, 300, R) * (rng.uniform(size=R) > 0.1)
    rows[:, 4] = rng.uniform(-5, 200, R) * (rng.uniform(size=R) > 0.1)
    rows[:, 5] = rng.standard_normal(R) * 3
    if image_form:
        return rows
    rows[:, 3] += rows[:, 1]
    rows[:, 4] += rows[:, 2]
    return rows.astype(np.float32)


def witness(rows, image_form, ratios):
    """The header's formulas: NET rows are copied; IMAGE rows: products (and x + w, y + h) in double, one rounding to fp32 each."""
    if not image_form:
        return rows[:, :5].copy(), rows.copy()
    img = rows[:, 0].astype(np.int64)
    rh = np.array([r[0] for r in ratios], np.float64)[img]
    rw = np.array([r[1] for r in ratios], np.float64)[img]
    props = np.stack([rows[:, 0].astype(np.float32), (rows[:, 1] * rw).astype(np.float32), (rows[:, 2] * rh).astype(np.float32),
                      ((rows[:, 1] + rows[:, 3]) * rw).astype(np.float32), ((rows[:, 2] + rows[:, 4]) * rh).astype(np.float32),
                      rows[:, 5].astype(np.float32)], axis=1)
    return props[:, :5].copy(), props


def check_good(hip, rows, image_form, N, with_props=True):
    ratios = [RATIOS[i % len(RATIOS)] for i in range(N)]
    rois, props, image_rows, status = hip.rois_ingest(dev(rows), hip.ROIS_IMAGE if image_form else hip.ROIS_NET, N,
                                                      ratios if image_form else None, with_props=with_props)
    want_rois, want_props = witness(rows, image_form, ratios)
    assert status.tolist() == [1, -1, 0, 0]
    assert np.array_equal(u32(rois), u32(want_rois))
    if with_props:
        assert np.array_equal(u32(props), u32(want_props))
    else:
        assert props is None
    assert image_rows.tolist() == np.bincount(rows[:, 0].astype(np.int64), minlength=N).tolist()


@pytest.mark.parametrize("image_form", [False, True])
@pytest.mark.parametrize("R", [1, 255, 256, 257])
def test_op_rows_around_the_step_size(hip, R, image_form):
    """256 rows per step: one row, one under, on and over a step; two images."""
    check_good(hip, synth_rows([R - R // 3, R // 3], 10 + R, image_form), image_form, 2)


@pytest.mark.parametrize("image_form", [False, True])
def test_op_an_image_without_rows_and_a_single_top(hip, image_form):
    rows = synth_rows([5, 0, 7], 3, image_form)
    check_good(hip, rows, image_form, 3)
    check_good(hip, rows, image_form, 3, with_props=False)      # props = NULL: a BoxOutput with one top
    check_good(hip, synth_rows([0, 0, 4], 4, image_form), image_form, 3)      # an empty FIRST image


def test_op_image_form_is_not_the_fp32_product(hip):
    """The data tells the double product rounded once from a product of fp32 numbers."""
    rows = synth_rows([300], 21, True)
    _, want = witness(rows, True, RATIOS[:1])
    alt = rows[:, 1].astype(np.float32) * np.float32(RATIOS[0][1])
    assert not np.array_equal(u32(alt), u32(want[:, 1]))
    check_good(hip, rows, True, 1)


BAD = [   # name, the row to spoil, how, the reason
    ("nan", 300, lambda rows, r, N: rows.__setitem__((r, 3), np.nan), 1),
    ("inf_score", 2, lambda rows, r, N: rows.__setitem__((r, 5), np.inf), 1),
    ("index_N", 300, lambda rows, r, N: rows.__setitem__((slice(r, None), 0), N), 2),
    ("index_fraction", 40, lambda rows, r, N: rows.__setitem__((r, 0), 0.5), 2),
    ("index_negative", 0, lambda rows, r, N: rows.__setitem__((r, 0), -1), 2),
    ("decreasing", 520, lambda rows, r, N: rows.__setitem__((r, 0), 0), 3),
]


@pytest.mark.parametrize("image_form", [False, True])
@pytest.mark.parametrize("name,row,spoil,reason", BAD)
def test_op_first_bad_row_and_reason(hip, name, row, spoil, reason, image_form):
    """600 rows in two images (image 1 from row 200 on).  The verdict names the first bad row; the rows of the steps in front of its step
    are written, nothing else (the wrapper pre-fills NaN / -1), and the launch ends cleanly."""
    N = 2
    rows = synth_rows([200, 400], 77, image_form)
    spoil(rows, row, N)
    ratios = [RATIOS[i] for i in range(N)]
    rois, props, image_rows, status = hip.rois_ingest(dev(rows), hip.ROIS_IMAGE if image_form else hip.ROIS_NET, N,
                                                      ratios if image_form else None)
    assert status.tolist() == [0, row, reason, 0], name
    done = row // 256 * 256
    good = rows[:done].copy()
    want_rois, want_props = witness(good, image_form, ratios)
    assert np.array_equal(u32(rois[:done]), u32(want_rois)) and np.array_equal(u32(props[:done]), u32(want_props))
    assert np.isnan(rois[done:]).all() and np.isnan(props[done:]).all() and image_rows.tolist() == [-1, -1]
    torch.cuda.synchronize()
    # one more bad row, at row 10: the verdict is that of whichever comes first
    rows[10, 1] = np.nan
    _, _, _, status = hip.rois_ingest(dev(rows), hip.ROIS_IMAGE if image_form else hip.ROIS_NET, N, ratios if image_form else None)
    assert status.tolist()[:3] == ([0, 0, 2] if name == "index_negative" else [0, 2, 1] if name == "inf_score" else [0, 10, 1])


def test_op_image_form_overflow_of_the_fp32_result_is_not_finite(hip):
    rows = synth_rows([20], 5, True)
    rows[7, 3] = 1e39      # finite in double, (x + w) * ratio_w past fp32's range
    _, _, _, status = hip.rois_ingest(dev(rows), hip.ROIS_IMAGE, 1, RATIOS[:1])
    assert status.tolist() == [0, 7, 1, 0]


# ---- the net entry -------------------------------------------------------------------------------------------------------------------
ORG_HW = (375, 1242)
KITTI = ("kitti_car/mscnn-7s-576", dict(height=96, width=320, max_nms_num=120))
CONFIGS = {   # model, reduced input, batch, classes, cascade, one-pass ROIAlign head
    "kitti_b1": KITTI + (1, [2], False, None),
    "kitti_b2": KITTI + (2, [2], False, None),
    "ped_cyc_2x": ("kitti_ped_cyc/mscnn-7s-576-2x", dict(height=192, width=448, max_nms_num=200), 1, [2, 3], False, None),
    "cascade_2x": ("kitti_car/cascade-mscnn-7s-576-2x", dict(height=192, width=448, max_nms_num=150), 1, [2], True, None),
    "align_off": ("widerface/cascade-mscnn-12s-align", dict(height=160, width=192, max_nms_num=150), 1, [2], True, False),
    "align_on": ("widerface/cascade-mscnn-12s-align", dict(height=160, width=192, max_nms_num=150), 1, [2], True, True),
}


def new_net(key):
    model, size, batch, _, _, one_pass = CONFIGS[key]
    n = mnet.Net(prototxt_text=zoo.prototxt(model, batch=batch, **size))
    ws = synth.load_into(n, "mid")
    if one_pass is not None:
        n.set_roialign_one_pass(one_pass)
    N, _, H, W = n.blob_shape("data")
    x = np.concatenate([synth.frame(H, W, seed=1701 + 13 * i, org_hw=ORG_HW) for i in range(N)], 0)
    params = [dict(ratios=(H / float(ORG_HW[0]), W / float(ORG_HW[1])), org_hw=ORG_HW) for _ in range(N)]
    return n, ws, x, params


def cascade_outputs(n):
    return [("output_bbox_1st", "cls_prob_1st", "proposals"), ("output_bbox_2nd", "cls_prob_2nd", "proposals_2nd"),
            ("output_bbox_3rd", "cls_prob_3rd_avg" if "cls_prob_3rd_avg" in n.blob_names else "cls_prob_3rd", "proposals_3rd")]


def final_stage(n, key, params):
    """Every detection of the frame as one flat list of (dets, ids), and the ROI counts."""
    _, _, _, classes, cascade, _ = CONFIGS[key]
    if cascade:
        per_image, rois = n.detect_cascade_multi(params, cascade_outputs(n), classes)
        return [seg for img in per_image for out in img for seg in out], rois
    per_image, rois = n.detect_multi(params, classes)
    return [seg for img in per_image for seg in img], rois


def subnet_blobs(n):
    """Every blob a layer from BoxOutput on writes: L's tops to the net's outputs, the ones a fusion leaves unwritten included."""
    L, _ = n.forward_rois_layers()
    names = []
    for i in range(L, len(n.layer_names)):
        names += [t for t in n.layer_tops(i) if t not in names]
    return names


def same_as_saved(n, key, params, saved, what):
    blobs, dets, rois = saved
    for name, ref in blobs.items():
        got = n.get_blob(name)
        assert got.shape == ref.shape, (what, name, got.shape, ref.shape)
        assert np.array_equal(u32(got), u32(ref)), (what, name)
    got_dets, got_rois = final_stage(n, key, params)
    assert got_rois == rois and len(got_dets) == len(dets), what
    for (d, i), (rd, ri) in zip(got_dets, dets):
        assert d.shape == rd.shape and np.array_equal(d.view(np.uint64), rd.view(np.uint64)) and np.array_equal(i, ri), what


_REF = {}


def reference_run(key):
    """One net per configuration after ONE whole forward on a fresh net, with everything that forward wrote saved."""
    if key not in _REF:
        n, ws, x, params = new_net(key)
        n.set_blob("data", x)
        n.forward()
        blobs = {name: n.get_blob(name) for name in subnet_blobs(n)}
        dets, rois = final_stage(n, key, params)
        _REF[key] = (n, ws, x, params, (blobs, dets, rois))
    return _REF[key]


@pytest.mark.parametrize("key", list(CONFIGS))
def test_round_trip_is_bit_identical(key):
    n, _, x, params, saved = reference_run(key)
    blobs = saved[0]
    ps = blobs["proposals_score"].reshape(-1, 6)
    R, N = len(ps), len(params)
    assert R > N and sum(len(d) for d, _ in saved[1]) > 0      # (a frame with something in it)
    assert "bbox_pred" in blobs and sum(name.startswith("roi_") for name in blobs) >= 3      # (the pooled / grid blobs of a fused head too)
    counts = np.bincount(ps[:, 0].astype(int), minlength=N).tolist()
    L, K = n.forward_rois_layers()
    skipped = n.layer_tops([i for i in range(K + 1, L) if n.layer_names[i].startswith("LFCN_")][0])[0]
    # the sub-net alone on the feature blobs of the forward just done
    assert n.forward_rois(ps, "net", run_trunk=False) == counts
    same_as_saved(n, key, params, saved, "run_trunk=0")
    # the trunk too: conv4_3 is spoilt first, a skipped layer's blob is marked -- the first comes back, the second stays
    n.set_blob("conv4_3", np.zeros(n.blob_shape("conv4_3"), np.float32))
    mark = np.full(n.blob_shape(skipped), 7.0, np.float32)
    n.set_blob(skipped, mark)
    assert n.forward_rois(dev(ps), "net", run_trunk=True) == counts      # (rows in device memory)
    same_as_saved(n, key, params, saved, "run_trunk=1")
    assert np.array_equal(n.get_blob(skipped), mark)
    # the same rows in original-image coordinates would be other numbers: not part of the round trip.  A whole forward afterwards is a
    # fresh net's
    n.forward()
    same_as_saved(n, key, params, saved, "forward() after forward_rois")
    assert not np.array_equal(n.get_blob(skipped), mark)


def test_first_call_on_a_net_and_the_numerics_watch():
    """forward_rois as the FIRST call on a net (BoxOutput has never run: its row bound comes from the bottoms' shapes), under a watch
    that would count every whole forward."""
    _, _, x, params, saved = reference_run("kitti_b1")
    ps = saved[0]["proposals_score"].reshape(-1, 6)
    n, _, _, _ = new_net("kitti_b1")
    n.set_numerics_watch(1)
    n.set_blob("data", x)
    assert n.forward_rois(ps, "net") == [len(ps)]
    assert n.numerics_watch_state()[0] == 0
    n.set_numerics_watch(25)
    same_as_saved(n, "kitti_b1", params, saved, "first call")
    n.forward()
    same_as_saved(n, "kitti_b1", params, saved, "forward() after a first forward_rois")


def test_row_bound_num_images_and_bad_rows():
    n, _, x, params, saved = reference_run("kitti_b1")
    ps = saved[0]["proposals_score"].reshape(-1, 6)
    cap = CONFIGS["kitti_b1"][1]["max_nms_num"]      # x 1 image
    rng = np.random.default_rng(5)
    rows = np.zeros((cap + 1, 6), np.float32)
    rows[:, 1] = rng.uniform(0, 250, cap + 1); rows[:, 2] = rng.uniform(0, 60, cap + 1)
    rows[:, 3] = rows[:, 1] + rng.uniform(4, 60, cap + 1); rows[:, 4] = rows[:, 2] + rng.uniform(4, 30, cap + 1)
    rows[:, 5] = rng.standard_normal(cap + 1)
    assert n.forward_rois(rows[:cap], "net", run_trunk=False) == [cap]
    assert n.blob_shape("proposals")[0] == cap and n.blob_shape("bbox_pred")[0] == cap and n.blob_shape("roi_pool")[0] == cap
    assert np.array_equal(u32(n.get_blob("proposals_score").reshape(-1, 6)), u32(rows[:cap]))
    segs, rois = n.detect_multi(params, [2])
    assert rois == [cap] and all(i < cap for i in segs[0][0][1])
    props, _ = n.proposals_multi(params)
    assert len(props[0][0]) == cap
    with pytest.raises(mnet.NetError, match=f"{cap + 1} rows, but BoxOutput layer proposals bounds a forward to {cap}"):
        n.forward_rois(rows, "net", run_trunk=False)
    with pytest.raises(mnet.NetError, match="num_images 2 but the net's input holds 1 images"):
        n.forward_rois(rows[:4], "net", num_images=2)
    with pytest.raises(mnet.NetError, match="R = 0"):
        n.forward_rois(rows[:0], "net")
    with pytest.raises(mnet.NetError, match="original-image coordinates need"):
        n.forward_rois(rows[:4].astype(np.float64), "image")
    assert n.blob_shape("proposals")[0] == cap      # nothing was touched by the refusals
    # a bad row fails the call naming row and reason; the sub-net is not run, and a forward afterwards is a fresh net's
    bad = rows[:50].copy()
    bad[31, 2] = np.nan
    with pytest.raises(mnet.NetError, match=r"row 31 of 50: a value that is not finite \(reason 1\).*sub-net was not run"):
        n.forward_rois(bad, "net", run_trunk=False)
    assert n.blob_shape("proposals") == (1, 5, 1, 1) and not n.get_blob("proposals_score").any()
    assert n.blob_shape("bbox_pred")[0] == cap
    bad = rows[:50].copy()
    bad[7, 0] = 1
    with pytest.raises(mnet.NetError, match=r"row 7 of 50: an image index outside \[0, num_images\)"):
        n.forward_rois(bad, "net")
    n.set_blob("data", x)
    n.forward()
    same_as_saved(n, "kitti_b1", params, saved, "forward() after refused and failed calls")
    assert n.forward_rois(ps, "net", run_trunk=False) == [len(ps)]
    same_as_saved(n, "kitti_b1", params, saved, "round trip after all that")


def test_arbitrary_rois_against_the_reference_layers():
    """About 40 boxes BoxOutput would never emit, in original-image coordinates on a batch of two: the ingested blobs are the header's
    formulas, ROI pooling is bit-exact against the reference's CPU layer on the device's feature blob, the sub-net within 1e-4 of the
    reference's layers on identical inputs (metric and bound of test_gpu_net.py steps (2) and (3)), the final stage selection-exact."""
    from oracle import pynet, pyoracle as orc, pyref
    from test_gpu_net import layer_list, rel_err
    backend = pyref if pyref.available() else None
    n, ws, x, params = new_net("kitti_b2")
    oh, ow = ORG_HW
    rng = np.random.default_rng(99)
    hand = [
        [0, 100.0, 50.0, 0.0, 80.0, 0.5],            # zero width
        [0, 100.0, 50.0, 80.0, 0.0, 0.25],           # zero height
        [0, -40.0, -20.0, 200.0, 150.0, 1.5],        # partly outside: left and top
        [0, ow - 60.0, oh - 30.0, 200.0, 100.0, 2.0],    # ... right and bottom
        [0, 400.0, 200.0, 1.0, 1.0, -1.0],           # one pixel
        [0, 0.0, 0.0, float(ow), float(oh), 3.0],    # the whole frame
        [0, 333.3, 111.1, 7.77, 213.9, 0.0],         # a sliver
    ]
    rows = []
    for i, extra in ((0, 14), (1, 19)):
        if i == 0:
            rows += hand
        r = np.zeros((extra, 6))
        r[:, 0] = i
        r[:, 1] = rng.uniform(0, ow - 50, extra); r[:, 2] = rng.uniform(0, oh - 30, extra)
        r[:, 3] = rng.uniform(8, 500, extra); r[:, 4] = rng.uniform(8, 250, extra)
        r[:, 5] = rng.standard_normal(extra) * 2
        rows += r.tolist()
    rows = np.asarray(rows, np.float64)
    R = len(rows)
    assert R == 40
    n.set_blob("data", x)
    assert n.forward_rois(rows, "image", params) == [21, 19]      # first call on the net, trunk included
    want_rois, want_props = witness(rows, True, [p["ratios"] for p in params])
    rois_dev = n.get_blob("proposals")
    assert rois_dev.shape == (R, 5, 1, 1)
    assert np.array_equal(u32(rois_dev.reshape(R, 5)), u32(want_rois))
    assert np.array_equal(u32(n.get_blob("proposals_score").reshape(R, 6)), u32(want_props))
    layers = layer_list(n)
    names = [l[0] for l in layers]
    parts = []
    for l in layers:
        if l[1] == "ROIPooling":
            parts.append(pynet.forward([l], ws, {l[2][0]: n.get_blob(l[2][0]), l[2][1]: rois_dev}, backend=backend)[l[3][0]])
            assert np.array_equal(n.get_blob(l[3][0]), parts[-1]), l[0]
    assert len(parts) == 2 and np.array_equal(n.get_blob("roi_pool"), np.concatenate(parts, axis=1))
    sub = layers[names.index("roi_pool") + 1:]
    r3 = pynet.forward(sub, ws, {"roi_pool": n.get_blob("roi_pool")}, backend=backend)
    for b in ("roi_c1", "fc6", "cls_pred", "bbox_pred"):
        e = rel_err(n.get_blob(b), r3[b])
        print(f"forward_rois sub-net {b}: rel_err {e:.3g}")
        assert e < 1e-4, (b, e)
    per_image, rois = n.detect_multi(params, [2])
    assert rois == [21, 19]
    bbox, cls, props = n.get_blob("bbox_pred"), n.get_blob("cls_pred"), n.get_blob("proposals_score").reshape(R, 6)
    total = 0
    for i in range(2):
        sel = np.flatnonzero(rows[:, 0] == i)
        dets, ids = per_image[i][0]
        dref, iref = orc.detections(bbox[sel], cls[sel], props[sel], cls_id=2, **params[i])
        assert np.array_equal(ids, sel[iref]), i
        assert rel_err(dets, dref) < 1e-4, i
        total += len(dets)
    assert total > 0


def test_driver_rois_in(tmp_path, capsys):
    """--rois-in on a small file (frame 2 of 3 has no rows): the detection file holds what Net.forward_rois + detect give on the
    parsed rows, per frame and per --batch group."""
    from mscnn_amd import kitti
    spec = importlib.util.spec_from_file_location("run_mscnn_detection", os.path.join(ROOT, "tools/run_mscnn_detection.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    model, size = KITTI
    text = zoo.prototxt(model, **size)
    deploy = tmp_path / "deploy.prototxt"
    deploy.write_text(text)
    rng = np.random.default_rng(8)
    per_frame = []
    for k in range(3):
        m = (12, 0, 9)[k]
        b = np.zeros((m, 5))
        b[:, 0] = rng.uniform(0, 1000, m); b[:, 1] = rng.uniform(0, 250, m)
        b[:, 2] = rng.uniform(30, 240, m); b[:, 3] = rng.uniform(30, 120, m); b[:, 4] = rng.standard_normal(m)
        per_frame.append(b)
    path = str(tmp_path / "rois.txt")
    kitti.write_detections_dlm(path, per_frame)
    parsed = drv.read_rois(path, 3)
    # what the calls give, frame by frame
    n = mnet.Net(prototxt_text=text)
    synth.load_into(n, "mid")
    H, W = n.blob_shape("data")[2:]
    want = []
    for k in range(1, 4):
        img = drv.load_frame(None, k)
        ratios = (H / float(img.shape[0]), W / float(img.shape[1]))
        if not len(parsed[k - 1]):
            continue
        n.set_image("data", torch.from_numpy(img).cuda())
        n.forward_rois(drv.group_rois([parsed[k - 1]]), "image", [dict(ratios=ratios)])
        dets, _, _ = n.detect(cls_id=2, ratios=ratios, org_hw=img.shape[:2])
        want += [[float("%.5g" % v) for v in [k] + list(d)] for d in dets]
    assert len(want) > 0 and {w[0] for w in want} <= {1.0, 3.0}
    for B in (1, 2):
        d = tmp_path / f"b{B}"
        assert drv.main(["--prototxt", str(deploy), "--synthetic", "3", "--out", str(d), "--comp-id", "t", "--cls-ids", "2", "--batch", str(B),
                         "--rois-in", path]) == 0
        got = kitti.read_detections_dlm(str(d / "t_car.txt"))
        if B == 1:
            assert got == want
        else:      # (a batched trunk is not bit-identical to a batch-1 trunk: the same detections within the file's precision)
            assert len(got) == len(want) and [g[0] for g in got] == [w[0] for w in want]
            assert np.allclose(np.asarray(got), np.asarray(want), rtol=1e-3, atol=1e-3)
    assert capsys.readouterr().out.count("idx 3/3, avgtime=") == 2
