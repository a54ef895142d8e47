"""Whole-net parity on the GPU: the C++ Caffe-compatible runtime (libmscnn_caffe.so -> libmscnn_hip.so) against the CPU
oracle, layer by layer with identical inputs (index-exact / 1e-4) and end to end by matched detections (SURVEY.md 7,
'Tolerance semantics')."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from mscnn_amd import net as mnet, synth, zoo   # noqa: E402


def layer_list(n):
    return [(n.layer_names[i], n.layer_types[i], n.layer_bottoms(i), n.layer_tops(i), n.layer_param_text(i)) for i in range(len(n.layer_names))]


_SCALE_METRIC = [False]      # check_net(scale_metric=True): hot activations, see rel_err


def rel_err(a, b):
    """max |a - b| / max(1, |b|), the metric of the reference's own tolerance (test_convolution_layer.cpp:256 on unit-scale data).
    With scale_metric the denominator is max(1, |b|, rms(b)): on blobs whose rms is far above 1 (the "vgg_like" regime: rms 10 .. 90)
    an element near zero is the difference of partial sums thousands of times its size, and ANY two fp32 summation orders --
    im2col + MKL against an MFMA chain, or the reference's own CPU against its GPU path -- differ there by more than 1e-4 of 1."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    if not a.size:
        return 0.0
    floor = max(1.0, float(np.sqrt((b ** 2).mean()))) if _SCALE_METRIC[0] else 1.0
    return float((np.abs(a - b) / np.maximum(floor, np.abs(b))).max())


def iou_xyxy(a, b):
    x1 = np.maximum(a[:, None, 0], b[None, :, 0]); y1 = np.maximum(a[:, None, 1], b[None, :, 1])
    x2 = np.minimum(a[:, None, 2], b[None, :, 2]); y2 = np.minimum(a[:, None, 3], b[None, :, 3])
    inter = np.clip(x2 - x1, 0, None) * np.clip(y2 - y1, 0, None)
    aa = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]); ab = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    return inter / (aa[:, None] + ab[None, :] - inter)


# reduced input sizes and a small top-K keep the CPU oracle (im2col + scalar GEMM) to seconds per config
CONFIGS = [
    ("kitti_car/mscnn-7s-576", dict(height=192, width=640, max_nms_num=300), "mid", 2),
    ("kitti_car/mscnn-8s-768-trainval", dict(height=128, width=384, max_nms_num=200), "dense", 2),
    ("kitti_ped_cyc/mscnn-7s-576-2x", dict(height=192, width=448, max_nms_num=200), "mid", 2),
    ("caltech/mscnn-7s-480", dict(height=240, width=320, max_nms_num=150), "mid", 2),
]

# BASELINE.json sizes: the deploy files' own input sizes and top-K (2000), every configuration the north star names, against
# oracle/_ref = the reference's own CPU layer sources (im2col + MKL sgemm; 20-60 s of host time per frame on the GPU box)
FULL_SIZE = [
    ("kitti_car/mscnn-7s-576", {}, "mid", 2, (375, 1242)),              # > 2000 anchors pass fg_thr: full top-K sort + NMS (the
                                                                        # "dense" weights select the same 2000, scores shifted)
    ("kitti_car/mscnn-7s-576", {}, "sparse", 2, (375, 1242)),           # fewer candidates than the top-K
    ("kitti_car/mscnn-7s-576", {}, "dense", 2, (375, 1242)),            # SURVEY 8(d) "dense": all 45,630 anchors pass fg_thr
    ("kitti_car/mscnn-7s-576", {"iou_thr": 1.01}, "mid", 2, (375, 1242)),   # no proposal suppressed: R = the top-K cap 2000, the sub-net's upper bound (bench.py regimes.max_rois)
    ("kitti_car/mscnn-8s-768-trainval", {}, "mid", 2, (375, 1242)),     # 1x3x768x2560, 8 heads, 81,600 anchors
    ("kitti_ped_cyc/mscnn-7s-576-2x", {}, "mid", 2, (375, 1242)),       # deconv 2x, 7x5 ROI pooling, fc6 2048
    ("caltech/mscnn-7s-480", {}, "mid", 2, (480, 640)),
]


def check_net(model, size, regime, cls_id, org_hw=(375, 1242), backend=None, precision=None, style="he", calibrate=False, scale_metric=False):
    _SCALE_METRIC[0] = bool(scale_metric)
    try:
        return _check_net(model, size, regime, cls_id, org_hw, backend, precision, style, calibrate)
    finally:
        _SCALE_METRIC[0] = False


def _check_net(model, size, regime, cls_id, org_hw, backend, precision, style, calibrate):
    from oracle import pynet, pyoracle as orc
    n = mnet.Net(prototxt_text=zoo.prototxt(model, **size))
    if precision:
        n.set_precision(precision)
    ws = synth.load_into(n, regime, style=style)
    H, W = n.blob_shape("data")[2:]
    x = synth.frame(H, W, org_hw=org_hw)
    n.set_blob("data", x)
    n.forward()
    layers = layer_list(n)
    report = {}
    if calibrate:      # the runtime's contract on unfamiliar statistics: Winograd layers off the direct sum on this data fall back
        errs, switched = n.calibrate_numerics(5e-5)
        report["calibration_fallbacks"] = switched
        report["calibration_max"] = float(max(errs.values(), default=0.0))
        n.forward()
    if precision:
        report["layers_" + precision] = sum(n.layer_dtype(i) == precision for i in range(len(n.layer_names)))
        assert report["layers_" + precision] >= 3, report

    # (1) end-to-end oracle run (its own intermediate values)
    ref = pynet.forward(layers, ws, {"data": x}, backend=backend)
    # trunk + heads: fp32 within 1e-4 relative
    for b in ("conv1_2", "conv2_2", "conv3_3", "conv4_3", "conv5_3", "conv6_1", "pool6"):
        report[b] = rel_err(n.get_blob(b), ref[b])
        assert report[b] < 1e-4, (b, report[b])
    head_tops = [t for (nm, ty, bo, to, _) in layers if nm.startswith("LFCN_") for t in to]
    for b in head_tops:
        report[b] = rel_err(n.get_blob(b), ref[b])
        assert report[b] < 1e-4, (b, report[b])

    # (2) per-layer, identical inputs: BoxOutput selection must be index-exact given the device's own head blobs
    heads_dev = [n.get_blob(b) for b in layers[[l[0] for l in layers].index("proposals")][2]]
    bo = [l for l in layers if l[1] == "BoxOutput"][0]
    r2 = pynet.forward([bo], ws, dict(zip(bo[2], heads_dev)), backend=backend)
    rois_dev = n.get_blob("proposals")
    R = rois_dev.shape[0]
    assert R == r2["proposals"].shape[0]
    assert np.array_equal(rois_dev, r2["proposals"])                      # bit-identical boxes and order
    assert np.array_equal(n.get_blob("proposals_score"), r2["proposals_score"])
    # ROI pooling on the device's feature map + ROIs: bit-exact.  The two ROIPooling layers write straight into the Concat
    # top (the Concat layer is fused away); their own tops are materialised lazily when somebody asks for them.
    assert n.fused_away(n.layer_names.index("roi_pool"))
    parts = []
    for l in layers:
        if l[1] == "ROIPooling":
            parts.append(pynet.forward([l], ws, {l[2][0]: n.get_blob(l[2][0]), l[2][1]: rois_dev}, backend=backend)[l[3][0]])
            assert np.array_equal(n.get_blob(l[3][0]), parts[-1]), l[0]      # roi_pool_org / roi_pool_ctx read back correctly
    assert np.array_equal(n.get_blob("roi_pool"), np.concatenate(parts, axis=1))
    if "conv4_3_2x" in n.blob_names:                                       # "-2x" nets: the bilinear Deconvolution
        l = [l for l in layers if l[1] == "Deconvolution"][0]
        d = pynet.forward([l], ws, {l[2][0]: n.get_blob(l[2][0])}, backend=backend)[l[3][0]]
        report["conv4_3_2x"] = rel_err(n.get_blob("conv4_3_2x"), d)
        assert report["conv4_3_2x"] < 1e-6
    # detection sub-net with identical inputs
    sub = layers[[l[0] for l in layers].index("roi_pool") + 1:]        # roi_c1 ... bbox_pred, incl. the auto-inserted Split
    feeds = {"roi_pool": n.get_blob("roi_pool")}
    r3 = pynet.forward(sub, ws, feeds, backend=backend)
    for b in ("roi_c1", "fc6", "cls_pred", "bbox_pred"):
        report["sub:" + b] = rel_err(n.get_blob(b), r3[b])
        assert report["sub:" + b] < 1e-4, (b, report["sub:" + b])

    # (3) final detection stage on the device outputs: selection exact, values 1e-4
    kw = dict(cls_id=cls_id, ratios=(H / float(org_hw[0]), W / float(org_hw[1])), org_hw=org_hw)
    dets, ids, Rd = n.detect(**kw)
    assert Rd == R
    dref, iref = orc.detections(n.get_blob("bbox_pred"), n.get_blob("cls_pred"), n.get_blob("proposals_score").reshape(R, 6), **kw)
    assert np.array_equal(ids, iref)
    assert rel_err(dets, dref) < 1e-4

    # (4) end to end vs the oracle's own run: matched detections (IoU >= 0.99, |dscore| <= 1e-4) -- candidates at the
    # fg_thr / top-K / IoU boundaries may legitimately flip because MFMA and CPU summation orders differ
    Rr = ref["proposals"].shape[0]
    de, ie = orc.detections(ref["bbox_pred"], ref["cls_pred"], ref["proposals_score"].reshape(Rr, 6), **kw)
    matched = None
    if len(de) and len(dets):
        a = np.stack([dets[:, 0], dets[:, 1], dets[:, 0] + dets[:, 2], dets[:, 1] + dets[:, 3]], 1)
        b = np.stack([de[:, 0], de[:, 1], de[:, 0] + de[:, 2], de[:, 1] + de[:, 3]], 1)
        m = iou_xyxy(a, b)
        j = m.argmax(1)
        matched = (m[np.arange(len(a)), j] >= 0.99) & (np.abs(dets[:, 4] - de[j, 4]) <= 1e-4)
        assert matched.mean() >= 0.98, f"only {matched.mean():.3f} of {len(a)} detections matched"
        # north star: "fp32 scores / boxes within 1e-4": the coordinates (x, y, w, h rows) of the matched pairs, reference metric
        # -- a corner is proposal corner + delta x std x proposal size: a bbox_pred 1.5e-5 off (its own gate: "sub:bbox_pred" above) moves
        # a 600-pixel box's corner by ~1e-3 px whatever the corner's own value, so the 1e-4 bound is taken against the box's extent and
        # the strict per-coordinate figure (a corner at x = 2 px of such a box) is held to 1e-3 and reported
        if matched.any():
            ref4 = de[j[matched], :4].astype(np.float64)
            dabs = np.abs(dets[matched, :4].astype(np.float64) - ref4)
            ext = np.maximum(1.0, np.maximum(np.abs(ref4).max(1), ref4[:, 2:4].max(1)))[:, None]
            report["dbox_max"] = float((dabs / np.maximum(1.0, np.abs(ref4))).max())
            report["dbox_vs_box_extent"] = float((dabs / ext).max())
            assert report["dbox_vs_box_extent"] < 1e-4 and report["dbox_max"] < 1e-3, (report["dbox_vs_box_extent"], report["dbox_max"])
    assert abs(len(de) - len(dets)) <= max(2, 0.02 * len(de))
    report.update(R=R, R_ref=Rr, dets=len(dets), dets_ref=len(de), matched=None if matched is None else float(matched.mean()))
    return report


@pytest.mark.parametrize("model,size,regime,cls_id", CONFIGS)
def test_net_layerwise_and_end_to_end(model, size, regime, cls_id):
    if not torch.cuda.is_available():
        pytest.fail("needs a MI355X")
    check_net(model, size, regime, cls_id)


@pytest.mark.parametrize("model,size,regime,cls_id", [CONFIGS[0], CONFIGS[2]])
def test_net_x3_precision_same_gates_as_fp32(model, size, regime, cls_id):
    """set_precision("f16x3") (split-fp16 Winograd GEMMs, max |x| handed from layer to layer on the device) is held to exactly
    the fp32 gates of check_net: per-layer 1e-4 against the oracle, selection layers bit-exact, >= 98 % matched detections."""
    if not torch.cuda.is_available():
        pytest.fail("needs a MI355X")
    rep = check_net(model, size, regime, cls_id, precision="f16x3")
    print("\nX3", model, {k: (f"{v:.1e}" if isinstance(v, float) else v) for k, v in rep.items()})


@pytest.mark.slow
@pytest.mark.parametrize("model,size,regime,cls_id,org_hw", [FULL_SIZE[0], FULL_SIZE[5]])
def test_full_size_parity_x3_vs_reference(model, size, regime, cls_id, org_hw):
    """The f16x3 mode at BASELINE sizes against the reference's own CPU layers, fp32 gates."""
    if not torch.cuda.is_available():
        pytest.fail("needs a MI355X")
    from oracle import pyref
    if not pyref.available():
        pytest.fail("oracle/_ref/libmscnn_ref.so did not travel to this box")
    rep = check_net(model, size, regime, cls_id, org_hw, backend=pyref, precision="f16x3")
    worst = max(v for k, v in rep.items() if isinstance(v, float) and k != "matched")
    print(f"\nFULLSIZE-X3 {model} {regime}: R {rep['R']}/{rep['R_ref']} dets {rep['dets']}/{rep['dets_ref']} matched {rep['matched']} "
          f"x3 layers {rep['layers_f16x3']} worst per-blob err {worst:.2e}")


@pytest.mark.slow
@pytest.mark.parametrize("model,size,regime,cls_id,org_hw", FULL_SIZE)
def test_full_size_parity_vs_reference(model, size, regime, cls_id, org_hw):
    """Every north-star configuration at ITS OWN input size and top-K against the reference's own CPU layers: the same
    assertions as the reduced-size test (per-layer 1e-4, BoxOutput / ROIPooling bit-exact on identical inputs, final-stage
    selection exact, >= 98 % matched detections end to end)."""
    if not torch.cuda.is_available():
        pytest.fail("needs a MI355X")
    from oracle import pyref
    if not pyref.available():
        pytest.fail("oracle/_ref/libmscnn_ref.so did not travel to this box (it is built by __graft_entry__.build() where "
                    "/root/reference exists and must not be listed in .gpurunignore)")
    rep = check_net(model, size, regime, cls_id, org_hw, backend=pyref)
    worst = max(v for k, v in rep.items() if isinstance(v, float) and k != "matched")
    print(f"\nFULLSIZE {model} {regime}: R {rep['R']}/{rep['R_ref']} dets {rep['dets']}/{rep['dets_ref']} matched {rep['matched']} "
          f"worst per-blob err {worst:.2e} " + " ".join(f"{k}={v:.1e}" for k, v in rep.items() if isinstance(v, float) and k != "matched"))


@pytest.mark.slow
def test_full_size_parity_vgg_like_weights():
    """Config 2 at its own size with the "vgg_like" weight statistics (tap sums not zero, log-normal filter gains, dead filters,
    biases, activations ~4x hotter than the He-normal regime; mscnn_amd/synth.py) against the reference's own CPU layers: after
    Net::CalibrateNumerics on the frame, the assertions of the He-normal test hold -- BoxOutput / ROIPooling bit-exact, final-stage
    selection exact, >= 98 % of the detections matched at IoU >= 0.99 and |dscore| <= 1e-4 -- with the per-blob bound taken relative
    to the blob's scale (rel_err with scale_metric: activations here have rms 10 .. 90)."""
    if not torch.cuda.is_available():
        pytest.fail("needs a MI355X")
    from oracle import pyref
    if not pyref.available():
        pytest.fail("oracle/_ref/libmscnn_ref.so did not travel to this box")
    rep = check_net("kitti_car/mscnn-7s-576", {}, "mid", 2, (375, 1242), backend=pyref, style="vgg_like", calibrate=True, scale_metric=True)
    worst = max(v for k, v in rep.items() if isinstance(v, float) and k not in ("matched", "calibration_max"))
    print(f"\nFULLSIZE-VGGLIKE R {rep['R']}/{rep['R_ref']} dets {rep['dets']}/{rep['dets_ref']} matched {rep['matched']} worst per-blob err "
          f"{worst:.2e}; calibration: max {rep['calibration_max']:.2e}, fall-backs {rep['calibration_fallbacks']}")


BATCHED = [   # model, reduced input, batch, original image size
    ("kitti_car/mscnn-7s-576", dict(height=192, width=640, max_nms_num=300), 2, (375, 1242)),
    ("kitti_car/mscnn-7s-576", dict(height=96, width=320, max_nms_num=120), 4, (375, 1242)),
    ("caltech/mscnn-7s-480", dict(height=240, width=320, max_nms_num=150), 4, (480, 640)),
    ("kitti_ped_cyc/mscnn-7s-576-2x", dict(height=192, width=448, max_nms_num=200), 2, (375, 1242)),
]


@pytest.mark.parametrize("model,size,batch,org_hw", BATCHED)
def test_whole_net_batch_n_vs_reference(model, size, batch, org_hw):
    """A `dim: N` forward of the whole net (the reference's path is batch-generic: conv_layer.cpp:25-40 loops over num_,
    box_output_layer.cpp:107 over images, roi_pooling_layer.cpp:62-66 reads the image from column 0 of every ROI) against the
    reference's own CPU layers run on the same N-image blob: trunk / heads 1e-4, BoxOutput (per image, rows grouped by image) and
    the ROI poolings over mixed images bit-exact on identical inputs, the detection sub-net (fused ROI pooling + roi_c1 over the
    ROIs of all images) 1e-4, and the final stage PER IMAGE (mscnn_net_detect_image) selection-exact against the oracle on that
    image's rows.  Also: mscnn_net_detect refuses the batched net, and every image's trunk agrees with its own batch-1 forward."""
    from oracle import pynet, pyoracle as orc, pyref
    backend = pyref if pyref.available() else None      # (the GPU box has oracle/_ref; without it the C restatement pinned to it)
    n = mnet.Net(prototxt_text=zoo.prototxt(model, batch=batch, **size))
    ws = synth.load_into(n, "mid")
    N, _, H, W = n.blob_shape("data")
    assert N == batch
    x = np.concatenate([synth.frame(H, W, seed=1701 + 13 * i, org_hw=org_hw) for i in range(N)], 0)
    n.set_blob("data", x)
    n.forward()
    layers = layer_list(n)
    names = [l[0] for l in layers]
    ref = pynet.forward(layers, ws, {"data": x}, backend=backend)
    for b in ("conv1_2", "conv3_3", "conv4_3", "conv5_3", "conv6_1", "pool6"):
        assert n.blob_shape(b)[0] == N
        assert rel_err(n.get_blob(b), ref[b]) < 1e-4, b
    for l in layers:
        if l[0].startswith("LFCN_"):
            assert rel_err(n.get_blob(l[3][0]), ref[l[3][0]]) < 1e-4, l[0]
    # BoxOutput on the device's own head blobs: bit-identical rows, grouped by image, every image present
    bo = [l for l in layers if l[1] == "BoxOutput"][0]
    r2 = pynet.forward([bo], ws, {b: n.get_blob(b) for b in bo[2]}, backend=backend)
    rois = n.get_blob("proposals")
    R = rois.shape[0]
    assert np.array_equal(rois, r2["proposals"]) and np.array_equal(n.get_blob("proposals_score"), r2["proposals_score"])
    img_of = rois.reshape(R, 5)[:, 0].astype(int)
    assert np.all(np.diff(img_of) >= 0) and set(img_of) == set(range(N)), np.bincount(img_of, minlength=N)
    # ROI poolings over mixed images (and the Deconvolution of the -2x nets in front of them)
    parts = []
    for l in layers:
        if l[1] == "ROIPooling":
            parts.append(pynet.forward([l], ws, {l[2][0]: n.get_blob(l[2][0]), l[2][1]: rois}, backend=backend)[l[3][0]])
            assert np.array_equal(n.get_blob(l[3][0]), parts[-1]), l[0]
    assert np.array_equal(n.get_blob("roi_pool"), np.concatenate(parts, axis=1))
    # the detection sub-net on the device's own ROI features
    sub = layers[names.index("roi_pool") + 1:]
    r3 = pynet.forward(sub, ws, {"roi_pool": n.get_blob("roi_pool")}, backend=backend)
    for b in ("roi_c1", "fc6", "cls_pred", "bbox_pred"):
        assert rel_err(n.get_blob(b), r3[b]) < 1e-4, b
    # final stage per image
    kw = dict(cls_id=2, ratios=(H / float(org_hw[0]), W / float(org_hw[1])), org_hw=org_hw)
    with pytest.raises(mnet.NetError, match="mscnn_net_detect_image"):
        n.detect(**kw)
    bbox, cls, props = n.get_blob("bbox_pred"), n.get_blob("cls_pred"), n.get_blob("proposals_score").reshape(R, 6)
    total = 0
    for i in range(N):
        rows = np.flatnonzero(img_of == i)
        dets, ids, Ri = n.detect_image(i, **kw)
        assert Ri == len(rows)
        dref, iref = orc.detections(bbox[rows], cls[rows], props[rows], **kw)
        assert np.array_equal(ids, rows[iref]) and rel_err(dets, dref) < 1e-4, i
        total += len(dets)
    assert total > 0
    # each image alone (batch 1 through the input-reshape entry of the same net): same trunk within the fp32 bar
    n.reshape_input("data", (1, 3, H, W))
    for i in (0, N - 1):
        n.set_blob("data", x[i:i + 1])
        n.forward()
        assert n.blob_shape("conv4_3")[0] == 1
        assert rel_err(n.get_blob("conv4_3"), ref["conv4_3"][i:i + 1]) < 1e-4
        assert rel_err(n.get_blob("conv6_1"), ref["conv6_1"][i:i + 1]) < 1e-4


def test_input_reshape_entry_equals_a_net_built_at_that_shape():
    """mscnn_net_reshape_input (blob->Reshape + Net::Reshape, net.cpp:743-747): a net built with `dim: 1` and reshaped to 3 images --
    and to another frame size -- is bit-identical, on every blob asked for, to a net built at that shape."""
    model, size = "kitti_car/mscnn-7s-576", dict(height=96, width=160, max_nms_num=100)
    a = mnet.Net(prototxt_text=zoo.prototxt(model, **size))
    synth.load_into(a, "mid")
    a.set_blob("data", synth.frame(96, 160))
    a.forward()
    for shape in ((3, 3, 96, 160), (2, 3, 128, 224), (1, 3, 96, 160)):
        b = mnet.Net(prototxt_text=zoo.prototxt(model, batch=shape[0], height=shape[2], width=shape[3], max_nms_num=100))
        synth.load_into(b, "mid")
        x = np.concatenate([synth.frame(shape[2], shape[3], seed=7 + i) for i in range(shape[0])], 0)
        a.reshape_input("data", shape)
        assert a.blob_shape("conv4_3")[0] == shape[0] and a.blob_shape("conv4_3")[2:] == (shape[2] // 8, shape[3] // 8)
        for m in (a, b):
            m.set_blob("data", x)
            m.forward()
        for blob in ("conv2_2", "conv4_3", "pool6", "proposals_score", "roi_pool", "fc6", "cls_pred", "bbox_pred"):
            assert np.array_equal(a.get_blob(blob), b.get_blob(blob)), (shape, blob)
    with pytest.raises(mnet.NetError, match="is not a net input"):
        a.reshape_input("conv4_3", (1, 512, 4, 4))


def test_caffemodel_file_drives_the_device_net(tmp_path):
    """SURVEY 8(f1) on the GPU: a .caffemodel written by the protobuf runtime (tests/caffemodel_pb.py: new-style, legacy 4-D and
    double_data blobs) is loaded into a DEVICE net through Net::CopyTrainedLayersFrom (net.cpp:750-803), forwarded on the HIP
    path, and compared blob by blob with the oracle run on the weights PARSED BACK FROM THE SAME FILE.  Also: the device net
    loaded from the file is bit-identical, on every blob, to one that received the same arrays through layer->blobs()."""
    from oracle import pynet
    from tests import caffemodel_pb
    model, size = "kitti_ped_cyc/mscnn-7s-576-2x", dict(height=96, width=160, max_nms_num=100)        # fc6 15.7 M weights (kitti_car: 52 M)
    n = mnet.Net(prototxt_text=zoo.prototxt(model, **size))
    shapes = [n.param_shapes(i) for i in range(len(n.layer_names))]
    ws = synth.weights(n.layer_names, n.layer_types, shapes, "mid")
    for name in ws:                                         # biases are zero in the synthetic regime: make the file carry real ones
        if len(ws[name]) > 1 and not name.startswith("LFCN_"):
            ws[name][1] = (0.05 * np.random.default_rng(len(name)).standard_normal(ws[name][1].shape)).astype(np.float32)
    modes = ["shape", "legacy", "double"]
    layers = [(name, n.layer_types[n.layer_names.index(name)], [(a, "shape" if a.size > 4_000_000 else modes[i % 3]) for a in arrs])
              for i, (name, arrs) in enumerate(ws.items())]
    path = tmp_path / "net.caffemodel"
    path.write_bytes(caffemodel_pb.serialize(layers))
    # weights as the FILE holds them (parsed by the protobuf runtime, not by our reader)
    back = caffemodel_pb.classes()["NetParameter"]()
    back.ParseFromString(path.read_bytes())
    ws_file = {}
    for lp in back.layer:
        arrs = []
        for bp, ref in zip(lp.blobs, ws[lp.name]):
            data = np.array(bp.double_data if len(bp.double_data) else bp.data, dtype=np.float32)
            arrs.append(data.reshape(ref.shape))
        ws_file[lp.name] = arrs
    n.load_caffemodel(path)
    x = synth.frame(96, 160)
    n.set_blob("data", x)
    n.forward()
    for name, arrs in ws_file.items():
        for p_, a in enumerate(arrs):
            assert np.array_equal(n.get_param(name, p_), a), (name, p_)
    # (a) against the oracle fed from the file
    layers_l = layer_list(n)
    ref = pynet.forward(layers_l, ws_file, {"data": x})
    checked = 0
    for b in n.blob_names:
        if b not in ref or "split" in b or b in ("proposals", "proposals_score"):
            continue
        g = n.get_blob(b)
        if g.shape != np.asarray(ref[b]).shape:
            continue                                        # ROI-count dependent blobs are compared below on identical inputs
        assert rel_err(g, ref[b]) < 1e-4, (b, rel_err(g, ref[b]))
        checked += 1
    assert checked >= 20, checked
    assert n.blob_shape("proposals")[0] == ref["proposals"].shape[0]
    # (b) against a device net that got the same arrays through set_param: identical bytes everywhere
    m = mnet.Net(prototxt_text=zoo.prototxt(model, **size))
    for name, arrs in ws_file.items():
        for p_, a in enumerate(arrs):
            m.set_param(name, p_, a)
    m.set_blob("data", x)
    m.forward()
    for b in n.blob_names:
        assert np.array_equal(n.get_blob(b), m.get_blob(b)), b
    dets_n, ids_n, _ = n.detect(cls_id=2, ratios=(96 / 375.0, 160 / 1242.0), org_hw=(375, 1242))
    dets_m, ids_m, _ = m.detect(cls_id=2, ratios=(96 / 375.0, 160 / 1242.0), org_hw=(375, 1242))
    assert np.array_equal(dets_n, dets_m) and np.array_equal(ids_n, ids_m)


def test_unfused_equals_fused():
    """Conv+ReLU fusion must be bit-identical to the separate layers (Layer API parity for stand-alone use)."""
    txt = zoo.prototxt("kitti_car/mscnn-7s-576", height=96, width=160)
    x = synth.frame(96, 160)
    outs = []
    for nofuse in ("0", "1"):
        n = mnet.Net(prototxt_text=txt, fusion=(nofuse == "0"))
        synth.load_into(n, "mid")
        n.set_blob("data", x)
        n.forward()
        assert n.fused_away(n.layer_names.index("relu1_1")) == (nofuse == "0")
        assert n.fused_away(n.layer_names.index("roi_pool")) == (nofuse == "0")
        outs.append({b: n.get_blob(b) for b in ("conv4_3", "conv6_1", "pool5", "proposals_score", "roi_pool_org", "roi_pool_ctx",
                                                 "roi_pool", "fc6", "bbox_pred")})
    for b in outs[0]:
        assert np.array_equal(outs[0][b], outs[1][b]), b


def test_partial_forward_over_fused_layers():
    """Net::ForwardFromTo with a range that starts after a fused layer's producer (net.cpp:544-555): the fused-away layer
    must recompute its top from its bottom, as the reference does, and a bottom reshaped between two Forward calls must
    propagate without Net::Reshape (layer.hpp:451-456)."""
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=96, width=160, max_nms_num=100))
    synth.load_into(n, "dense")
    n.set_blob("data", synth.frame(96, 160))
    n.forward()
    want = {b: n.get_blob(b) for b in ("pool1", "pool4", "roi_pool", "fc6", "cls_pred")}
    names = n.layer_names
    # (a) clobber a fused Pooling layer's top, run the net from that layer on: it must be rebuilt from conv1_2
    i = names.index("pool1")
    assert n.fused_away(i)
    n.set_blob("pool1", np.full(n.blob_shape("pool1"), 7.0, np.float32))
    n.forward(i, i)
    assert np.array_equal(n.get_blob("pool1"), want["pool1"])
    # (b) from a fused in-place ReLU on: idempotent on the already rectified blob
    n.forward(names.index("relu4_3"), len(names) - 1)
    for b in ("roi_pool", "fc6", "cls_pred"):
        assert np.array_equal(n.get_blob(b), want[b]), b
    # (c) from the fused Concat on: its bottoms live inside the Concat top and are materialised first
    n.set_blob("roi_pool", np.zeros(n.blob_shape("roi_pool"), np.float32))
    n.forward(names.index("roi_pool_ctx"), names.index("roi_pool_ctx"))       # re-run one producer: writes its window
    n.forward(names.index("roi_pool_org"), names.index("roi_pool_org"))
    n.forward(names.index("roi_pool"), len(names) - 1)
    for b in ("roi_pool", "fc6", "cls_pred"):
        assert np.array_equal(n.get_blob(b), want[b]), b


def test_handoff_timeout_never_hands_out_a_wrong_frame():
    """The stream-K hand-off of the plane-GEMM kernel under fault injection (contributors never publish, mscnn_hip.h:
    mscnn_debug_wgemm_handoff_fault), at the Net level: whatever the layer, the frame that comes out of the C ABI is the correct one and
    the event is counted (mscnn_net_handoff_state).
      (a) a time-out in the TRUNK: its NaN head scores would be dropped by BoxOutput without a trace -- the Net sees the status word
          behind BoxOutput's own synchronisation, forces whole tiles and restarts the range inside the same Forward;
      (b) a time-out behind BoxOutput (roi_c1): seen behind the final stage's synchronisation (mscnn_net_detect), frame run again;
      (c) the same through mscnn_net_get_blob."""
    from mscnn_amd import hipapi as hip
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=192, width=640, max_nms_num=300))
    synth.load_into(n, "mid")
    n.set_blob("data", synth.frame(192, 640))
    kw = dict(cls_id=2, ratios=(192 / 375.0, 640 / 1242.0), org_hw=(375, 1242))
    blobs = ("conv2_2", "conv4_3", "conv6_1", "proposals_score", "roi_c1", "fc6", "cls_pred", "bbox_pred")
    convs = [i for i, t in enumerate(n.layer_types) if t == "Convolution"]
    try:
        # the truth: every launch on whole tiles (first forward: the layers' own first-input checks run and pass)
        hip.wgemm_force_whole_tiles(True)
        n.forward()
        assert n.auto_calibrate_state()[1] == []
        n.forward()
        want = {b: n.get_blob(b) for b in blobs}
        want_dets = n.detect(**kw)
        hip.wgemm_force_whole_tiles(False)
        assert n.handoff_state() == (0, False)
        wino = [i for i in convs if n.layer_kernel(i).startswith("winograd")]
        assert len(wino) >= 8 and n.layer_names.index("roi_c1") in wino

        # (a) every Winograd layer splits its tiles, nobody publishes
        for i in wino:
            n.set_conv_tuning(i, 300 + 256)
        n.forward()                                        # (healthy split run: no event, same frame within the split's tolerance)
        assert n.handoff_state() == (0, False)
        assert rel_err(n.get_blob("cls_pred"), want["cls_pred"]) < 1e-4
        hip.debug_wgemm_handoff_fault(True, 64)
        n.forward()
        dets = n.detect(**kw)
        assert n.handoff_state() == (1, True)
        for b in blobs:
            assert np.array_equal(n.get_blob(b), want[b]), b
        assert all(np.array_equal(u, v) for u, v in zip(dets, want_dets))
        assert n.handoff_state() == (1, True)              # (nothing is split any more: nothing more to report)

        # (b) only roi_c1 splits: the event lies behind BoxOutput and is answered by the final stage
        hip.wgemm_force_whole_tiles(False)
        for i in wino:
            n.set_conv_tuning(i, 300 + (256 if n.layer_names[i] == "roi_c1" else 512))
        n.forward()
        assert n.handoff_state() == (1, False)             # not looked at yet: no synchronisation point since roi_c1 ran
        dets = n.detect(**kw)
        assert n.handoff_state() == (2, True)
        assert all(np.array_equal(u, v) for u, v in zip(dets, want_dets))

        # (c) ... or by a blob read
        hip.wgemm_force_whole_tiles(False)
        n.forward()
        got = n.get_blob("cls_pred")
        assert n.handoff_state() == (3, True)
        assert np.array_equal(got, want["cls_pred"])
        assert np.array_equal(n.get_blob("roi_c1"), want["roi_c1"])
    finally:
        hip.debug_wgemm_handoff_fault(False, 0)
        hip.wgemm_force_whole_tiles(False)


def test_zero_warmup_frame_does_not_use_up_the_first_forward_check():
    """an all-zero warm-up frame makes the Winograd-vs-direct comparison of the first forward empty (both forms return the
    bias); the layers' checks must stay armed and run on the first frame that carries data."""
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=96, width=160, max_nms_num=100))
    synth.load_into(n, "mid")
    n.set_blob("data", np.zeros(n.blob_shape("data"), np.float32))
    n.forward()
    checks0, switched0, _ = n.auto_calibrate_state()
    n.set_blob("data", synth.frame(96, 160))
    n.forward()
    checks1, switched1, errs = n.auto_calibrate_state()
    wino = [i for i, t in enumerate(n.layer_types) if t == "Convolution" and n.layer_kernel(i).startswith("winograd")]
    # conv1_2 sees a zero bottom on the zero frame (conv1_1 has no bias in the synthetic regime) -- at least that check was deferred;
    # after the real frame every Winograd layer has been checked exactly once
    assert checks0 < len(wino) and checks1 == len(wino), (checks0, checks1, len(wino))
    assert switched1 == [] and 0 < max(errs.values()) < 5e-5
    n.forward()
    assert n.auto_calibrate_state()[0] == checks1


def test_numerical_calibration_falls_back_per_layer():
    """Net::CalibrateNumerics: Winograd layers are compared with the direct kernel on the current input; with an impossible
    tolerance every one of them must fall back (and the net must still agree with itself), with the default one none does."""
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=192, width=384, max_nms_num=100))
    synth.load_into(n, "mid")
    n.set_blob("data", synth.frame(192, 384))
    n.forward()
    before = {b: n.get_blob(b) for b in ("conv4_3", "conv5_3", "fc6")}
    wino = [nm for i, nm in enumerate(n.layer_names) if n.layer_kernel(i).startswith("winograd")]
    assert "conv4_2" in wino and "roi_c1" in wino
    errs, switched = n.calibrate_numerics(5e-5)
    assert sorted(errs) == sorted(wino) and switched == [] and 0 < max(errs.values()) < 5e-5, errs
    errs, switched = n.calibrate_numerics(1e-9)
    assert sorted(switched) == sorted(wino)
    n.forward()
    assert not any(n.layer_kernel(i).startswith("winograd") for i in range(len(n.layer_names)))
    for b, v in before.items():
        assert rel_err(n.get_blob(b), v) < 1e-4, b


def test_numerics_watch_rechecks_one_layer_per_period_on_live_frames():
    """mscnn_net_set_numerics_watch: every period-th whole forward re-computes one Winograd layer (round robin) with the direct
    kernel on the live frame.  Default tolerance: checks happen, nothing is switched, outputs unchanged; impossible tolerance: the
    layers leave Winograd one per period, in net order."""
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=192, width=384, max_nms_num=100))
    synth.load_into(n, "mid")
    wino = lambda: [nm for i, nm in enumerate(n.layer_names) if n.layer_kernel(i).startswith("winograd")]      # noqa: E731
    n.set_blob("data", synth.frame(192, 384))
    n.forward()
    w0 = wino()
    ref = n.get_blob("fc6")
    assert n.numerics_watch_state() == (0, [])
    n.set_numerics_watch(2, 5e-5)
    for _ in range(2 * len(w0) + 1):
        n.forward()
    checks, switched = n.numerics_watch_state()
    assert checks == len(w0) and switched == [] and wino() == w0
    assert np.array_equal(n.get_blob("fc6"), ref)
    n.set_numerics_watch(1, 1e-9)
    for k in range(3):
        n.set_blob("data", synth.frame(192, 384, seed=5 + k))
        n.forward()
    checks, switched = n.numerics_watch_state()
    assert checks == len(w0) + 3 and len(switched) == 3 and set(switched) <= set(w0)
    assert wino() == [nm for nm in w0 if nm not in switched]
    n.set_numerics_watch(0)
    n.forward()
    assert n.numerics_watch_state()[0] == checks


def test_numerics_watch_moves_each_layer_to_its_next_band():
    """the watch compared band 0 of every layer on every visit.  Each layer now goes round its own bands, one per visit:
    on one fixed frame, the second trip round the Winograd layers measures other rows / ROIs than the first, so most layers with
    two or more bands (a map of >= 32 rows, or several images / ROIs) report another error on their second visit."""
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=192, width=384, max_nms_num=100))
    synth.load_into(n, "mid")
    n.set_blob("data", synth.frame(192, 384))
    n.forward()
    wino = [i for i, t in enumerate(n.layer_types) if t == "Convolution" and n.layer_kernel(i).startswith("winograd")]
    shape = lambda i: n.blob_shape(n.layer_bottoms(i)[0])      # noqa: E731
    banded = [i for i in wino if shape(i)[2] >= 32 or shape(i)[0] >= 2]
    n.set_numerics_watch(1, 1.0)
    seen = {i: [] for i in wino}
    for k in range(2 * len(wino)):      # round robin in net order: check k looks at wino[k % len(wino)]
        n.forward()
        assert n.numerics_watch_state() == (k + 1, [])
        i = wino[k % len(wino)]
        seen[i].append(mnet.lib().mscnn_net_layer_calibration_err(n._h, i))
    moved = [n.layer_names[i] for i in banded if seen[i][0] != seen[i][1]]
    assert len(banded) >= 4 and len(moved) > len(banded) // 2, (moved, [n.layer_names[i] for i in banded], seen)


WINO_STACK = 'name: "wino_stack"\ninput: "data" input_dim: 1 input_dim: 128 input_dim: 32 input_dim: 64\n' + "".join(
    'layer { name: "c%d" type: "Convolution" bottom: "%s" top: "c%d" convolution_param { num_output: 128 pad: 1 kernel_size: 3 '
    'weight_filler { type: "gaussian" std: 0.03 } } }\n' % (k, "data" if k == 0 else "c%d" % (k - 1), k) for k in range(12))


def test_numerics_watch_checks_any_number_of_layer_instances():
    """every layer ever band-checked kept one word of a 1024-word pinned array per (thread, device) for good, so after about
    1024 layer instances (~80 model reloads) every watch frame failed.  Each layer now owns its verdict record: nets of twelve Winograd
    layers are built, watched once per layer and destroyed, well past 1024 layer instances."""
    x = np.random.default_rng(7).standard_normal((1, 128, 32, 64)).astype(np.float32)
    total = 0
    while total <= 1100:
        n = mnet.Net(prototxt_text=WINO_STACK)
        n.set_numerics_watch(1, 1.0)
        n.set_blob("data", x)
        n.forward()      # (plans the layers: the watch looks at planned Winograd layers)
        L = sum(n.layer_kernel(i).startswith("winograd") for i in range(len(n.layer_names)))
        assert L == 12, [n.layer_kernel(i) for i in range(len(n.layer_names))]
        for _ in range(L):
            n.forward()
        assert n.numerics_watch_state() == (L, [])
        total += L
        del n


def test_dynamic_roi_count_across_forwards():
    """R changes from image to image; Reshape propagation (layer.hpp:451-456) must follow without reallocating downwards."""
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=128, width=256))
    synth.load_into(n, "mid")
    seen = set()
    for seed in (1, 2, 3):
        n.set_blob("data", synth.frame(128, 256, seed=seed))
        n.forward()
        R = n.blob_shape("proposals")[0]
        assert n.blob_shape("roi_pool") == (R, 1024, 7, 7) and n.blob_shape("bbox_pred") == (R, 20)
        seen.add(R)
    n.set_blob("data", np.zeros((1, 3, 128, 256), np.float32))   # nothing like an object -> may hit few/no proposals
    n.forward()
    assert n.blob_shape("cls_pred")[0] == n.blob_shape("proposals")[0] >= 1


MINI_CASCADE = """
name: "mini_cascade"
input: "data" input_dim: 1 input_dim: 3 input_dim: 96 input_dim: 160
layer { name: "conv1_1" type: "Convolution" bottom: "data" top: "conv1_1" convolution_param { num_output: 16 pad: 1 kernel_size: 3 } }
layer { name: "relu1_1" type: "ReLU" bottom: "conv1_1" top: "conv1_1" }
layer { name: "pool1" type: "Pooling" bottom: "conv1_1" top: "pool1" pooling_param { pool: MAX kernel_size: 2 stride: 2 } }
layer { name: "conv2_1" type: "Convolution" bottom: "pool1" top: "conv2_1" convolution_param { num_output: 32 pad: 1 kernel_size: 3 } }
layer { name: "relu2_1" type: "ReLU" bottom: "conv2_1" top: "conv2_1" }
layer { name: "pool2" type: "Pooling" bottom: "conv2_1" top: "pool2" pooling_param { pool: MAX kernel_size: 2 stride: 2 } }
layer { name: "conv3_1" type: "Convolution" bottom: "pool2" top: "conv3_1" convolution_param { num_output: 32 pad: 1 kernel_size: 3 } }
layer { name: "relu3_1" type: "ReLU" bottom: "conv3_1" top: "conv3_1" }
layer { name: "LFCN_1_5x5" type: "Convolution" bottom: "conv3_1" top: "LFCN_1_5x5" convolution_param { num_output: 6 pad: 2 kernel_size: 5 } }
layer { name: "proposals" type: "BoxOutput" bottom: "LFCN_1_5x5" top: "proposals" top: "proposals_score"
        box_output_param { fg_thr: -3 iou_thr: 0.65 nms_type: "IOU" field_w: 24 field_h: 24 downsample_rate: 4 max_nms_num: 60 min_size: 4 } }
layer { name: "roi_align" type: "ROIAlign" bottom: "conv3_1" bottom: "proposals" top: "roi_align"
        roi_pooling_param { pooled_w: 6 pooled_h: 6 spatial_scale: 0.25 pad_ratio: 0 } }
layer { name: "roi_align_ave" type: "Pooling" bottom: "roi_align" top: "roi_align_ave" pooling_param { pool: AVE kernel_size: 2 stride: 1 } }
layer { name: "fc_a" type: "InnerProduct" bottom: "roi_align_ave" top: "fc_a" inner_product_param { num_output: 64 } }
layer { name: "relu_a" type: "ReLU" bottom: "fc_a" top: "fc_a" }
layer { name: "cls_1st" type: "InnerProduct" bottom: "fc_a" top: "cls_1st" inner_product_param { num_output: 2 } }
layer { name: "bbox_1st" type: "InnerProduct" bottom: "fc_a" top: "bbox_1st" inner_product_param { num_output: 8 } }
layer { name: "proposals_2nd" type: "DecodeBBox" bottom: "bbox_1st" bottom: "proposals" top: "proposals_2nd"
        bbox_reg_param { bbox_mean: 0 bbox_mean: 0 bbox_mean: 0 bbox_mean: 0 bbox_std: 0.1 bbox_std: 0.1 bbox_std: 0.2 bbox_std: 0.2 } }
layer { name: "roi_pool_2nd" type: "ROIPooling" bottom: "conv3_1" bottom: "proposals_2nd" top: "roi_pool_2nd"
        roi_pooling_param { pooled_w: 4 pooled_h: 4 spatial_scale: 0.25 pad_ratio: 0.25 } }
layer { name: "fc_b" type: "InnerProduct" bottom: "roi_pool_2nd" top: "fc_b" inner_product_param { num_output: 64 } }
layer { name: "relu_b" type: "ReLU" bottom: "fc_b" top: "fc_b" }
layer { name: "cls_2nd" type: "InnerProduct" bottom: "fc_b" top: "cls_2nd" inner_product_param { num_output: 2 } }
layer { name: "cls_prob_1st" type: "Softmax" bottom: "cls_1st" top: "cls_prob_1st" }
layer { name: "cls_prob_2nd" type: "Softmax" bottom: "cls_2nd" top: "cls_prob_2nd" }
layer { name: "cls_prob_avg" type: "Eltwise" bottom: "cls_prob_1st" bottom: "cls_prob_2nd" top: "cls_prob_avg"
        eltwise_param { operation: SUM coeff: 0.5 coeff: 0.5 } }
"""


def test_cascade_style_net():
    """The layer chain of the cascade / WiderFace deploys (DecodeBBox -> re-pooling, ROIAlign + 2x2 AVE pooling, Softmax,
    Eltwise) on a small hand-written net: per-layer parity with identical inputs."""
    from oracle import pynet
    n = mnet.Net(prototxt_text=MINI_CASCADE)
    ws = synth.load_into(n, "dense")
    x = synth.frame(96, 160)
    n.set_blob("data", x)
    n.forward()
    layers = layer_list(n)
    assert n.outputs == ["cls_prob_avg", "proposals_score"]
    R = n.blob_shape("proposals")[0]
    assert R > 3 and n.blob_shape("roi_align") == (R, 32, 7, 7) and n.blob_shape("roi_align_ave") == (R, 32, 6, 6)
    names = [l[0] for l in layers]
    relu_inplace = {l[2][0] for l in layers if l[1] == "ReLU" and l[2] == l[3]}
    # every layer after the trunk: feed the oracle with the device's own bottoms, compare the top
    for l in layers[names.index("proposals"):]:
        if l[1] in ("Split",):
            continue
        feeds = {b: n.get_blob(b) for b in l[2]}
        ref = pynet.forward([l], ws, feeds)
        for t in l[3]:
            a, b = n.get_blob(t), ref[t].reshape(n.blob_shape(t))
            if t in relu_inplace and l[1] != "ReLU":
                b = np.maximum(b, 0)        # the device blob has already been through its in-place ReLU
            if l[1] in ("BoxOutput", "ROIAlign", "ROIPooling", "DecodeBBox", "Eltwise", "ReLU"):
                assert np.array_equal(a, b), (l[0], t)
            else:
                assert rel_err(a, b) < 1e-4, (l[0], t)
    # and the trunk end to end
    ref = pynet.forward(layers[:names.index("proposals")], ws, {"data": x})
    assert rel_err(n.get_blob("LFCN_1_5x5"), ref["LFCN_1_5x5"]) < 1e-4


CASCADES = [   # model, reduced input, cls_id, original image size
    ("kitti_car/cascade-mscnn-7s-576-2x", dict(height=192, width=448, max_nms_num=150), 2, (375, 1242)),
    ("citypersons/mscnn-8s-1344-2x", dict(height=256, width=384, max_nms_num=150), 2, (1024, 2048)),
    ("citypersons/cascade-mscnn-8s-1344-2x", dict(height=256, width=384, max_nms_num=150), 2, (1024, 2048)),
    ("widerface/cascade-mscnn-12s-align", dict(height=160, width=192, max_nms_num=150), 2, (600, 720)),
]


@pytest.mark.parametrize("model,size,cls_id,org_hw,precision",
                         [c + (None,) for c in CASCADES] + [CASCADES[0] + ("f16x3",), CASCADES[3] + ("f16x3",)])
def test_cascade_deploys_whole_net(model, size, cls_id, org_hw, precision):
    _check_cascade(model, size, cls_id, org_hw, precision)


@pytest.mark.slow
def test_cascade_full_size_vs_reference():
    """kitti_car/cascade-mscnn-7s-576-2x at the deploy file's own size (1x3x576x1920, 2x up-sampled conv4_3, three detection
    stages, max_nms_num 2000) against the reference's own CPU layers (oracle/_ref): the assertions of the reduced-size test."""
    if not torch.cuda.is_available():
        pytest.fail("needs a MI355X")
    from oracle import pyref
    if not pyref.available():
        pytest.fail("oracle/_ref/libmscnn_ref.so did not travel to this box")
    _check_cascade("kitti_car/cascade-mscnn-7s-576-2x", {}, 2, (375, 1242), None, backend=pyref)


def _check_cascade(model, size, cls_id, org_hw, precision, backend=None):
    """The reference's cascade / CityPersons / WiderFace deploy nets (the generated prototxts are checked against the shipped
    files in tests/test_prototxt.py) forwarded on the GPU: trunk + heads end to end within 1e-4 of the oracle, then EVERY layer
    from BoxOutput on with the device's own bottoms (DecodeBBox chains, stage-wise re-pooling, ROIAlign + AVE pooling, the
    third-stage ensemble, Softmax, Eltwise) bit-exact for selection / sampling layers and 1e-4 for GEMM layers, and the cascade
    drivers' final stage (run_cascademscnn.m:84-127) on each cascade output against its oracle.  precision "f16x3": the same
    assertions with the split-fp16 kernels (every stage's roi_c1 / fc6 included)."""
    from oracle import pynet, pyoracle as orc
    n = mnet.Net(prototxt_text=zoo.prototxt(model, **size))
    if precision:
        n.set_precision(precision)
    ws = synth.load_into(n, "mid")
    H, W = n.blob_shape("data")[2:]
    x = synth.frame(H, W)
    n.set_blob("data", x)
    n.forward()
    layers = layer_list(n)
    names = [l[0] for l in layers]
    ip = names.index("proposals")
    ref = pynet.forward(layers[:ip], ws, {"data": x}, backend=backend)
    f16 = precision == "f16"      # the fp16 policy: GEMM layers within 1e-2 of the blob's rms, everything else as in fp32

    def gemm_ok(a, b):
        if not f16:
            return rel_err(a, b) < 1e-4
        a = np.asarray(a, np.float64); b = np.asarray(b, np.float64).reshape(a.shape)
        return float(np.abs(a - b).max() / max(np.sqrt((b ** 2).mean()), 1e-6)) < 1e-2
    for l in layers[:ip]:
        if l[0].startswith("LFCN_") or l[0] in ("conv4_3", "conv5_3", "pool6"):
            assert gemm_ok(n.get_blob(l[3][0]), ref[l[3][0]]), l[0]
    R = n.blob_shape("proposals")[0]
    assert R > 8, R
    if precision:
        assert sum(n.layer_dtype(i) == precision for i in range(len(n.layer_names))) >= 6
    relu_inplace = {l[2][0] for l in layers if l[1] == "ReLU" and l[2] == l[3]}
    for l in layers[ip:]:
        if l[1] in ("Split", "ReLU", "Dropout"):
            continue
        feeds = {b: n.get_blob(b) for b in l[2]}
        out = pynet.forward([l], ws, feeds, backend=backend)
        for t in l[3]:
            a, b = n.get_blob(t), out[t].reshape(n.blob_shape(t))
            if t in relu_inplace:
                b = np.maximum(b, 0)        # the device blob has already been through its (fused) in-place ReLU
            if l[1] in ("BoxOutput", "ROIAlign", "ROIPooling", "DecodeBBox", "Eltwise", "Concat"):
                assert np.array_equal(a, b), (l[0], t)
            elif l[1] == "Pooling" and "AVE" in l[4]:
                assert rel_err(a, b) < 1e-6, (l[0], t)
            elif l[1] in ("Convolution", "InnerProduct"):
                assert gemm_ok(a, b), (l[0], t)
            else:
                assert rel_err(a, b) < 1e-4, (l[0], t)
    # the cascade drivers' final stage on every cascade output of this net
    kw = dict(cls_id=cls_id, ratios=(H / float(org_hw[0]), W / float(org_hw[1])), org_hw=org_hw)
    outs = [("output_bbox_1st", "cls_prob_1st", "proposals"), ("output_bbox_2nd", "cls_prob_2nd", "proposals_2nd"),
            ("output_bbox_3rd", "cls_prob_3rd_avg" if "cls_prob_3rd_avg" in n.blob_names else "cls_prob_3rd", "proposals_3rd")]
    seen = 0
    for bb, pb, qb in outs:
        if bb not in n.blob_names:
            continue
        dets, ids, Rd = n.detect_cascade(bb, pb, qb, det_thr=0.0, **kw)
        Rr = n.blob_shape(bb)[0]
        dref, iref = orc.detections_cascade(n.get_blob(bb).reshape(Rr, 5), n.get_blob(pb).reshape(Rr, -1), n.get_blob(qb).reshape(Rr, 5), **kw)
        assert Rd == Rr and np.array_equal(ids, iref) and np.array_equal(dets, dref), bb
        seen += 1
    assert seen == (3 if "proposals_3rd" in n.blob_names else 1)


def _match_fraction(dets, dref, iou_min, dscore):
    if len(dets) == 0 or len(dref) == 0:
        return 1.0 if len(dets) == len(dref) else 0.0
    a = np.stack([dets[:, 0], dets[:, 1], dets[:, 0] + dets[:, 2], dets[:, 1] + dets[:, 3]], 1)
    b = np.stack([dref[:, 0], dref[:, 1], dref[:, 0] + dref[:, 2], dref[:, 1] + dref[:, 3]], 1)
    m = iou_xyxy(a, b)
    j = m.argmax(1)
    return float(((m[np.arange(len(a)), j] >= iou_min) & (np.abs(dets[:, 4] - dref[j, 4]) <= dscore)).mean())


@pytest.mark.parametrize("model,size,org_hw", [("caltech/mscnn-7s-480", dict(height=240, width=320, max_nms_num=300), (480, 640)),
                                                ("kitti_car/mscnn-7s-576", dict(height=192, width=640, max_nms_num=300), (375, 1242))])
def test_f16_precision_mode_tolerance_policy(model, size, org_hw):
    """BASELINE config 5 (fp16 MFMA convolutions; the reference has no counterpart, include/caffe/common.hpp:41-44).  Policy:
    (a) every trunk / sub-net blob within 1e-2 of the fp32 HIP path AND of the CPU oracle, relative to the blob's rms;
    (b) final detections against the fp32 HIP path and against the oracle's own run: >= 95 % matched at IoU >= 0.95 with
        |dscore| <= 5e-3, detection counts within 5 %;
    (c) the integer / selection layers stay exact given identical inputs (BoxOutput on the fp16 net's own head blobs)."""
    _check_f16_policy(model, size, org_hw, None)


@pytest.mark.slow
def test_full_size_f16_caltech_vs_reference():
    """BASELINE configs[4] at ITS OWN size and precision: examples/caltech/mscnn-7s-480/mscnn_deploy.prototxt (1 x 3 x 480 x 640, top-K
    2000) in the fp16 MFMA mode, the fp16 tolerance policy above asserted against the reference's own CPU layers (oracle/_ref) --
    every kernel the fp16 net runs at the size the config names (chains, pool-only stores, the 8 x 4 ROI pooling + roi_c1, fc6)."""
    if not torch.cuda.is_available():
        pytest.fail("needs a MI355X")
    from oracle import pyref
    if not pyref.available():
        pytest.fail("oracle/_ref/libmscnn_ref.so did not travel to this box")
    _check_f16_policy("caltech/mscnn-7s-480", {}, (480, 640), pyref)


@pytest.mark.slow
@pytest.mark.parametrize("precision", [None, "f16"])
def test_full_size_citypersons_640x480_vs_reference(precision):
    """The other net BASELINE configs[4] names: the CityPersons deploy (examples/citypersons/mscnn-8s-1344-2x/mscnn_deploy.prototxt:
    8 heads, BoxOutput with bbox_reg normalisation, Deconvolution 2x, 8 x 4 ROI pooling, DecodeBBox + Softmax outputs) on a 640 x 480
    stream frame with the deploy file's own top-K, against the reference's own CPU layers: fp32 under the 1e-4 / bit-exact gates of the
    cascade test, fp16 under the fp16 policy (GEMM layers 1e-2 of the blob's rms on identical inputs, selection / sampling layers
    still bit-exact, final stage exact on the device's own outputs)."""
    if not torch.cuda.is_available():
        pytest.fail("needs a MI355X")
    from oracle import pyref
    if not pyref.available():
        pytest.fail("oracle/_ref/libmscnn_ref.so did not travel to this box")
    _check_cascade("citypersons/mscnn-8s-1344-2x", dict(height=480, width=640), 2, (480, 640), precision, backend=pyref)


def _check_f16_policy(model, size, org_hw, backend):
    from oracle import pynet, pyoracle as orc
    txt = zoo.prototxt(model, **size)
    x = None
    nets = {}
    for dt in ("f32", "f16"):
        n = mnet.Net(prototxt_text=txt)
        ws = synth.load_into(n, "mid")
        n.set_precision(dt)
        if x is None:
            H, W = n.blob_shape("data")[2:]
            x = synth.frame(H, W, org_hw=org_hw)
            kw = dict(cls_id=2, ratios=(H / float(org_hw[0]), W / float(org_hw[1])), org_hw=org_hw)
        n.set_blob("data", x)
        n.forward()
        nets[dt] = n
    n32, n16 = nets["f32"], nets["f16"]
    names = n16.layer_names
    conv16 = [nm for i, nm in enumerate(names) if n16.layer_dtype(i) == "f16"]
    assert {"conv1_2", "conv4_2", "conv5_3", "conv6_1", "roi_c1", "fc6"} <= set(conv16), conv16
    assert all(n16.layer_dtype(names.index(nm)) == "f32" for nm in names if nm.startswith("LFCN_") or nm in ("cls_pred", "bbox_pred"))
    assert all(n32.layer_dtype(i) == "f32" for i in range(len(names)))
    layers = layer_list(n16)
    ref = pynet.forward(layers, ws, {"data": x}, backend=backend)

    def rms_err(a, b):
        a = np.asarray(a, np.float64); b = np.asarray(b, np.float64).reshape(a.shape)
        return float(np.abs(a - b).max() / max(np.sqrt((b ** 2).mean()), 1e-6))
    for b in ("conv1_2", "conv2_2", "conv3_3", "conv4_3", "conv5_3", "conv6_1"):
        e32, eor = rms_err(n16.get_blob(b), n32.get_blob(b)), rms_err(n16.get_blob(b), ref[b])
        assert e32 < 1e-2 and eor < 1e-2, (b, e32, eor)
    # (c) selection exact on identical inputs
    bo = [l for l in layers if l[1] == "BoxOutput"][0]
    r2 = pynet.forward([bo], ws, {b: n16.get_blob(b) for b in bo[2]}, backend=backend)
    assert np.array_equal(n16.get_blob("proposals"), r2["proposals"])
    # sub-net on the fp16 net's own ROI features: fp16 roi_c1 / fc6 against the oracle
    sub = layers[[l[0] for l in layers].index("roi_pool") + 1:]
    r3 = pynet.forward(sub, ws, {"roi_pool": n16.get_blob("roi_pool")}, backend=backend)
    for b in ("roi_c1", "fc6", "cls_pred", "bbox_pred"):
        assert rms_err(n16.get_blob(b), r3[b]) < 1e-2, b
    # (b) detections
    d16, _, R16 = n16.detect(**kw)
    d32, _, R32 = n32.detect(**kw)
    Rr = ref["proposals"].shape[0]
    dor, _ = orc.detections(ref["bbox_pred"], ref["cls_pred"], ref["proposals_score"].reshape(Rr, 6), **kw)
    for name, dref in (("fp32 HIP path", d32), ("CPU oracle", dor)):
        frac = _match_fraction(d16, dref, 0.95, 5e-3)
        print(f"f16 vs {name}: {len(d16)} / {len(dref)} detections, matched {frac:.3f}")
        assert frac >= 0.95, (name, frac)
        assert abs(len(d16) - len(dref)) <= max(2, 0.05 * len(dref)), name


def test_set_image_preprocessing():
    """Net-level pre-processing (run_mscnn_detection.m:64-69 on the device): a 375x1242-like uint8 RGB frame -> the input blob,
    bit-identical to the oracle's restatement, from host memory and from a device tensor."""
    from oracle import pyoracle as orc
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=192, width=640))
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (125, 414, 3), dtype=np.uint8)
    ref = orc.preprocess(img, 192, 640)
    n.set_image("data", img)
    assert np.array_equal(n.get_blob("data"), ref)
    n.set_image("data", torch.from_numpy(img[::-1].copy()).cuda(), mean_bgr=(100.0, 110.0, 120.0))
    assert np.array_equal(n.get_blob("data"), orc.preprocess(img[::-1].copy(), 192, 640, mean_bgr=(100.0, 110.0, 120.0)))


def test_reference_style_user_code_runs_on_the_gpu(tmp_path):
    """The drop-in boundary, executed: tests/boundary/run_boundary.cpp -- the reference's SyncedMemory test cases
    (test_syncedmem.cpp:13-120), Blob semantics, and a Net whose prototxt names two user-registered layer types (one binds
    the C ABI inside Forward_gpu the way INTEGRATION.md section 1 shows, one uses only the Layer / Blob interface) beside the
    stock ROIPooling: the user layer must produce the stock layer's bytes."""
    import subprocess
    from tests.test_cabi import build_boundary_binary
    exe = build_boundary_binary(tmp_path)
    r = subprocess.run([exe, str(tmp_path / "boundary.prototxt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("BOUNDARY OK"), (r.stdout[-1000:], r.stderr[-2000:])


def test_generated_deploys_match_the_fingerprints_of_the_shipped_files():
    """What the GPU box forwards are the reference's deploy files: every generated net (mscnn_amd/zoo.py), built on the device,
    hashes to the fingerprint tests/golden/make_deploy_fingerprints.py took from the shipped mscnn_deploy.prototxt of the same
    name (graph, blob shapes, outputs, every TEST-phase parameter) -- the reference checkout itself is not on this box."""
    import json
    from deploy_fingerprint import fingerprint
    want = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deploy_fingerprints.json")))
    assert sorted(want) == sorted(zoo.MODELS)
    for model in sorted(zoo.MODELS):
        n = mnet.Net(prototxt_text=zoo.prototxt(model))
        assert fingerprint(n) == want[model]["sha256"], model
        del n



def _read_f32(path):
    raw = np.fromfile(path, np.int32, 1)
    nd = int(raw[0])
    shape = np.fromfile(path, np.int32, 1 + nd)[1:]
    return np.fromfile(path, np.float32, offset=4 * (1 + nd)).reshape(tuple(int(v) for v in shape))


def test_default_flow_is_safe_without_a_calibration_call(tmp_path):
    """the INTEGRATION.md section 2 flow -- Net(prototxt, TEST); CopyTrainedLayersFrom(file); Forward() -- as a C++
    program against the mirror headers (tests/boundary/run_default_flow.cpp), with heavy-tailed weights in the .caffemodel and NO
    calibration call anywhere.  (a) default settings: every Winograd layer has checked itself on that first frame, and the blobs the
    program wrote meet the parity gates against the oracle run on the same file's weights; (b) with the documented knob set to an
    impossible tolerance every Winograd layer must have fallen back INSIDE that first Forward: the program's blobs are bit-identical
    to a net whose convolutions were all forced onto the direct kernel."""
    if not torch.cuda.is_available():
        pytest.fail("needs a MI355X")
    import subprocess
    from oracle import pynet
    from tests import caffemodel_pb
    from tests.test_cabi import build_boundary_binary
    model, size = "kitti_ped_cyc/mscnn-7s-576-2x", dict(height=192, width=320, max_nms_num=100)
    proto = zoo.prototxt(model, **size)
    n = mnet.Net(prototxt_text=proto)
    shapes = [n.param_shapes(i) for i in range(len(n.layer_names))]
    ws = synth.weights(n.layer_names, n.layer_types, shapes, "mid", style="heavy_tailed")
    (tmp_path / "deploy.prototxt").write_text(proto)
    (tmp_path / "net.caffemodel").write_bytes(caffemodel_pb.serialize(
        [(name, n.layer_types[n.layer_names.index(name)], [(a, "shape") for a in arrs]) for name, arrs in ws.items()]))
    x = synth.frame(192, 320)
    x.tofile(str(tmp_path / "input.f32"))
    exe = build_boundary_binary(tmp_path, "run_default_flow.cpp")

    def run(outdir, *extra):
        os.makedirs(outdir)
        r = subprocess.run([exe, str(tmp_path / "deploy.prototxt"), str(tmp_path / "net.caffemodel"), str(tmp_path / "input.f32"), outdir, *extra],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "DEFAULT FLOW OK" in r.stdout, (r.stdout[-1500:], r.stderr[-2500:])
        kern = {l.split()[1]: l.split()[2] for l in r.stdout.splitlines() if l.startswith("LAYER ")}
        checked = [l.split()[1] for l in r.stdout.splitlines() if l.startswith("LAYER ") and float(l.split()[3]) > 0]
        cal = [l for l in r.stdout.splitlines() if l.startswith("AUTOCAL")][0].split()
        assert int(cal[2]) == len(checked)
        return kern, checked, int(cal[4])

    # (a) defaults
    kern, checked, switched = run(str(tmp_path / "a"))
    wino_left = [k for k, v in kern.items() if v.startswith("winograd")]
    print(f"\nDEFAULT-FLOW heavy_tailed: {len(checked)} first-forward checks, {switched} fall-backs, Winograd left on {wino_left}")
    assert len(checked) >= 4 and len(checked) == switched + len(wino_left), (checked, switched, kern)
    ref = pynet.forward(layer_list(n), ws, {"data": x})
    _SCALE_METRIC[0] = True
    try:
        for b in ("conv2_2", "conv3_3", "conv4_3", "conv5_3", "conv6_1", "LFCN_1_5x7", "LFCN_3_3x5"):
            e = rel_err(_read_f32(str(tmp_path / "a" / (b + ".f32"))), ref[b])
            assert e < 1e-4, (b, e)
    finally:
        _SCALE_METRIC[0] = False
    assert _read_f32(str(tmp_path / "a" / "proposals.f32")).shape[0] == ref["proposals"].shape[0]
    # (b) the knob: impossible tolerance => all-direct, decided and recomputed within the first Forward
    kern_b, checked_b, switched_b = run(str(tmp_path / "b"), "1e-12")
    assert checked_b == checked and switched_b == len(checked) and not any(v.startswith("winograd") for v in kern_b.values()), kern_b
    n.set_auto_calibrate(0.0)                                   # the opt-out: nothing is checked ...
    for name, arrs in ws.items():
        for p_, a in enumerate(arrs):
            n.set_param(name, p_, a)
    for name in checked:                                        # ... and the layers AUTO would run as Winograd forced onto the direct kernel
        n.set_conv_algo(name, 1)
    n.set_blob("data", x)
    n.forward()
    assert n.auto_calibrate_state()[0] == 0
    for b in ("conv2_2", "conv4_3", "conv6_1", "LFCN_2_5x7", "proposals", "roi_pool", "fc6", "cls_pred", "bbox_pred"):
        assert np.array_equal(_read_f32(str(tmp_path / "b" / (b + ".f32"))), n.get_blob(b)), b


def test_roi_pooling_deferred_into_roi_c1():
    """Round 4: the ROIPooling pair's blob has one reader, roi_c1, whose Winograd input stage pools straight from the feature map
    (mscnn_conv2d_fwd_roipool_pair_f32): the blob is not written during Forward, and still (a) every blob behind it is bit-identical
    to the net without fusion, (b) asking for roi_pool / roi_pool_org / roi_pool_ctx by name yields the reference's bytes (written on
    demand), (c) a partial range that rewrites conv4_3 without re-running the pooling first saves the pending blob, (d) a plan that
    cannot fuse (f16x3 mode) falls back to the written blob."""
    txt = zoo.prototxt("kitti_car/mscnn-7s-576", height=192, width=640, max_nms_num=300)
    x = synth.frame(192, 640)
    n = mnet.Net(prototxt_text=txt)
    u = mnet.Net(prototxt_text=txt, fusion=False)
    for net in (n, u):
        synth.load_into(net, "mid")
        net.set_blob("data", x)
        net.forward()
        net.forward()                                    # (the first forward ran the layers' own numerical checks on the written blob)
    names = n.layer_names
    i_c1 = names.index("roi_c1")
    assert n.layer_kernel(i_c1) == "winograd_f3x3_3x3+roipool_pair" and u.layer_kernel(i_c1) == "winograd_f3x3_3x3"
    assert n.blob_shape("proposals")[0] >= 8
    for b in ("roi_c1", "fc6", "cls_pred", "bbox_pred"):
        assert np.array_equal(n.get_blob(b), u.get_blob(b)), b
    for b in ("roi_pool_org", "roi_pool", "roi_pool_ctx"):      # (b) on demand
        assert np.array_equal(n.get_blob(b), u.get_blob(b)), b
    # (c) pending again after a new forward; then conv1_1 .. conv4_3 of ANOTHER frame without the pooling layers: roi_pool must still
    # be the first frame's, as in the reference where the blob was written when the layer ran
    n.forward()
    want = u.get_blob("roi_pool")
    n.set_blob("data", synth.frame(192, 640, seed=77))
    n.forward(0, names.index("relu4_3"))
    assert not np.array_equal(n.get_blob("conv4_3"), u.get_blob("conv4_3"))
    assert np.array_equal(n.get_blob("roi_pool"), want)
    # ... and writing a blob the pending pooling reads (C ABI setter) does the same
    n.set_blob("data", x)
    n.forward()
    n.set_blob("conv4_3", np.zeros(n.blob_shape("conv4_3"), np.float32))
    assert np.array_equal(n.get_blob("roi_pool"), want)
    # (d) f16x3: the split-fp16 plan has its own input transform -> the blob is written and read
    n.set_blob("data", x)
    n.set_precision("f16x3")
    n.forward()
    n.forward()
    assert not n.layer_kernel(i_c1).endswith("+roipool_pair")
    u.set_precision("f16x3")
    u.forward()
    assert np.array_equal(n.get_blob("fc6"), u.get_blob("fc6"))


def test_convolution_chains_keep_every_blob_bit_identical():
    """Round 4: conv2_1 -> conv2_2, conv3_1 -> 3_2 -> 3_3, conv4_1 -> 4_2 -> 4_3 run as chains (mscnn_conv2d_fwd_chain_f32): the blob
    between two members is not written during a forward.  (a) every blob of the net -- the skipped ones re-created on demand -- is
    bit-identical to the net with the chains off; (b) the skipped blobs really were skipped (kernel name) and detections agree; (c) a
    partial range that starts at a consumer runs from the blob; (d) a partial range that rewrites a chain's bottom does not change
    what a skipped blob of the EARLIER frame reads as; (e) writing such a bottom through the ABI neither."""
    # (full size: AUTO takes F(4x4,3x3) only where the map has >= 1000 tiles)
    txt = zoo.prototxt("kitti_car/mscnn-7s-576")
    x = synth.frame(576, 1920)
    n = mnet.Net(prototxt_text=txt)
    u = mnet.Net(prototxt_text=txt)
    u.set_chain_fusion(False)
    for net in (n, u):
        synth.load_into(net, "mid")
        net.set_blob("data", x)
        net.forward()
        net.forward()                                    # (the first forward ran the layers' own numerical checks, unchained)
    names = n.layer_names
    producers = ["conv2_1", "conv3_1", "conv3_2", "conv4_1", "conv4_2"]
    for p in producers:
        assert n.layer_kernel(names.index(p)) == "winograd_f4x4_3x3+into_next", (p, n.layer_kernel(names.index(p)))
        assert u.layer_kernel(names.index(p)) == "winograd_f4x4_3x3"
    for t in ("conv2_2", "conv3_3", "conv4_3"):      # (conv2_2 / conv3_3 write their pooled blob only: read by the fused pooling alone)
        assert n.layer_kernel(names.index(t)) == "winograd_f4x4_3x3"
    # (a) tails and everything behind them first (no re-creation involved), then the skipped blobs
    for b in ("pool2", "conv3_3", "conv4_3", "conv5_3", "fc6", "cls_pred", "bbox_pred", "proposals"):
        assert np.array_equal(n.get_blob(b), u.get_blob(b)), b
    for b in producers[::-1] + ["conv2_2", "conv1_2"]:
        assert np.array_equal(n.get_blob(b), u.get_blob(b)), b
    # (c) from conv3_2 on, with a conv3_1 blob written from outside: both nets compute the same from it
    z = (u.get_blob("conv3_1") * 0.5).astype(np.float32)
    for net in (n, u):
        net.forward()
        net.set_blob("conv3_1", z)
        net.forward(names.index("conv3_2"), names.index("relu4_3"))
    assert np.array_equal(n.get_blob("conv4_3"), u.get_blob("conv4_3"))
    assert np.array_equal(n.get_blob("conv3_2"), u.get_blob("conv3_2"))
    # (d) a whole forward, then conv1_1 .. pool2 of ANOTHER frame: conv3_1 / conv3_2 still read as the first frame's
    for net in (n, u):
        net.set_blob("data", x)
        net.forward()
    want31, want32 = u.get_blob("conv3_1"), u.get_blob("conv3_2")
    for net in (n, u):
        net.set_blob("data", synth.frame(576, 1920, seed=77))
        net.forward(0, names.index("pool2"))
    assert not np.array_equal(n.get_blob("pool2"), np.zeros(1)) and np.array_equal(n.get_blob("pool2"), u.get_blob("pool2"))
    assert np.array_equal(n.get_blob("conv3_2"), want32) and np.array_equal(n.get_blob("conv3_1"), want31)
    # (e) the same through a setter
    n.set_blob("data", x)
    n.forward()
    n.set_blob("pool2", np.zeros(n.blob_shape("pool2"), np.float32))
    assert np.array_equal(n.get_blob("conv3_2"), want32) and np.array_equal(n.get_blob("conv3_1"), want31)
    # (f) changing a weight after a forward does not change what the skipped blobs of THAT forward read as
    n.set_blob("data", x)
    n.forward()
    w32 = n.get_param("conv3_2", 0)
    n.set_param("conv3_2", 0, (w32 * 0.5).astype(np.float32))
    assert np.array_equal(n.get_blob("conv3_2"), want32) and np.array_equal(n.get_blob("conv3_1"), want31)
    n.set_param("conv3_2", 0, w32)
    n.forward()      # (first forward after a weight change: conv3_2 checks itself, unchained)
    # detections of the chained net = the unchained net's (whole frames)
    kw = dict(cls_id=2, ratios=(576 / 375.0, 1920 / 1242.0), org_hw=(375, 1242))
    for net in (n, u):
        net.set_blob("data", x)
        net.forward()
    dn, du = n.detect(**kw), u.detect(**kw)
    assert dn[0].tobytes() == du[0].tobytes() and np.array_equal(dn[1], du[1]) and len(dn[0]) > 0


def test_detect_begin_end_pipelined_is_bit_identical_to_detect():
    """mscnn_net_detect_begin / _end (round 6): the final stage of a STREAM of frames -- frame i's pack is copied to pinned memory
    behind an event while the caller already forwards frame i + 1 -- hands out exactly what the blocking mscnn_net_detect returns for
    the same frames (detections, ROI rows, R), in order, with two frames in flight; a third begin and an end with nothing in flight
    are refused by name."""
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=192, width=448, max_nms_num=300))
    synth.load_into(n, "mid")
    H, W = n.blob_shape("data")[2:]
    kw = dict(cls_id=2, ratios=(H / 375.0, W / 1242.0), org_hw=(375, 1242))
    frames = [synth.frame(H, W, seed=40 + i) for i in range(4)]
    want = []
    for f in frames:
        n.set_blob("data", f)
        n.forward()
        want.append(n.detect(**kw))
    assert len({w[2] for w in want}) > 1 and all(len(w[0]) > 0 for w in want)      # different ROI counts frame to frame
    cap = 300
    got = []
    for i, f in enumerate(frames):
        n.set_blob("data", f)
        n.forward()
        n.detect_begin(cap, **kw)
        if i >= 1:
            got.append(n.detect_end(cap))                       # frame i - 1, collected after frame i was enqueued
    with pytest.raises(mnet.NetError, match="nothing in flight|in flight"):
        n.detect_end(cap); n.detect_end(cap)                    # the second one has nothing left
    assert len(got) == 3
    n.set_blob("data", frames[3]); n.forward(); n.detect_begin(cap, **kw)
    n.set_blob("data", frames[0]); n.forward(); n.detect_begin(cap, **kw)
    with pytest.raises(mnet.NetError, match="two frames already in flight"):
        n.detect_begin(cap, **kw)
    got.append(n.detect_end(cap))
    last = n.detect_end(cap)
    for (d, ids, R), (dw, iw, Rw) in zip(got + [last], want + [want[0]]):
        assert R == Rw and np.array_equal(ids, iw) and np.array_equal(d, dw)


@pytest.mark.slow
@pytest.mark.parametrize("model,size,org_hw", [("kitti_car/mscnn-7s-576", dict(height=288, width=960, max_nms_num=600), (375, 1242)),
                                               ("caltech/mscnn-7s-480", dict(height=240, width=320, max_nms_num=150), (480, 640))])
def test_stream_of_frames_fused_host_machinery_is_bit_identical_to_the_eager_net(model, size, org_hw):
    """A soak of the host-side machinery of round 6 over a stream of DIFFERENT frames (the ROI count changes every frame): the default Net
    -- ROI maps built under BoxOutput's round trip from the previous frame's decision, the row count and the detection pack written into
    host-coherent memory by the kernels, convolution chains, the numerics watch every 3rd frame (producers keeping their tops, a band
    check in flight behind every third frame) and the pipelined final stage on every other frame -- must hand out, frame by frame,
    exactly the detections, ROI rows and blobs of an eager net (fusion off, watch off) fed the same frames.  Stale state of any of
    these (maps of an earlier frame, a count read too early, a pack slot reused, a top left unwritten) would show as a difference."""
    txt = zoo.prototxt(model, **size)
    a = mnet.Net(prototxt_text=txt)
    b = mnet.Net(prototxt_text=txt, fusion=False)
    synth.load_into(a, "mid"); synth.load_into(b, "mid")
    b.set_numerics_watch(0)
    a.set_numerics_watch(3, 5e-5)
    H, W = a.blob_shape("data")[2:]
    kw = dict(cls_id=2, ratios=(H / float(org_hw[0]), W / float(org_hw[1])), org_hw=org_hw)
    cap = size["max_nms_num"]
    frames = [synth.frame(H, W, seed=300 + i, org_hw=org_hw) for i in range(24)]
    frames[7] = np.zeros_like(frames[0])                                 # a frame with nothing in it (the dummy-row path) in the middle
    want = []
    for f in frames:
        b.set_blob("data", f)
        b.forward()
        want.append((b.detect(**kw), b.get_blob("proposals"), b.get_blob("fc6")))
    assert len({w[0][2] for w in want}) >= 5                              # the ROI count really varies
    pending = None
    for i, f in enumerate(frames):
        a.set_blob("data", f)
        a.forward()
        if i % 2 == 0:
            got = a.detect(**kw)
        else:                                                            # pipelined: collect right away (one in flight)
            a.detect_begin(cap, **kw)
            got = a.detect_end(cap)
        (dw, iw, Rw), pw, fw = want[i]
        assert got[2] == Rw and np.array_equal(got[1], iw) and np.array_equal(got[0], dw), (i, got[2], Rw)
        if i % 5 == 0:                                                   # blobs, some of them re-created on demand in the fused net
            assert np.array_equal(a.get_blob("proposals"), pw) and np.array_equal(a.get_blob("fc6"), fw), i
    checks, switched = a.numerics_watch_state()
    assert checks >= 6 and switched == []


def test_net_final_stage_above_4032_rois_keeps_the_device_pack_path():
    """mscnn_net_detect writes its pack straight into host-coherent memory up to 4032 ROIs (round 6); above that -- the tiled sort / NMS
    path of the final stage -- the pack stays on the device and is copied.  A reduced 7s-576 net with max_nms_num 5000 and iou_thr 1.01
    in the dense regime hands more than 4032 ROIs to the sub-net: BoxOutput (its own tiled path) bit-exact against the oracle on the
    device's head blobs, the final stage index-exact against the oracle on the device's outputs, and a second call (the host buffer
    re-used after a larger frame) equal to the first."""
    from oracle import pynet, pyoracle as orc
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=192, width=640, max_nms_num=5000, iou_thr=1.01, min_size=1))
    ws = synth.load_into(n, "dense")
    H, W = n.blob_shape("data")[2:]
    x = synth.frame(H, W, seed=77)
    n.set_blob("data", x)
    n.forward()
    R = n.blob_shape("proposals")[0]
    assert R > 4032, R
    layers = layer_list(n)
    bo = [l for l in layers if l[1] == "BoxOutput"][0]
    r2 = pynet.forward([bo], ws, {b: n.get_blob(b) for b in bo[2]})
    assert np.array_equal(n.get_blob("proposals"), r2["proposals"]) and np.array_equal(n.get_blob("proposals_score"), r2["proposals_score"])
    kw = dict(cls_id=2, ratios=(H / 375.0, W / 1242.0), org_hw=(375, 1242))
    dets, ids, Rd = n.detect(cap=8192, **kw)
    dref, iref = orc.detections(n.get_blob("bbox_pred"), n.get_blob("cls_pred"), n.get_blob("proposals_score").reshape(R, 6), **kw)
    assert Rd == R and np.array_equal(ids, iref) and rel_err(dets, dref) < 1e-4
    # a frame with few ROIs next (the sparse heads: the host-coherent path), then the large one again
    synth.set_regime(n, "sparse")
    n.set_blob("data", x); n.forward()
    d0, i0, R0 = n.detect(cap=8192, **kw)
    assert 1 <= R0 <= 4032, R0
    dr0, ir0 = orc.detections(n.get_blob("bbox_pred"), n.get_blob("cls_pred"), n.get_blob("proposals_score").reshape(R0, 6), **kw)
    assert np.array_equal(i0, ir0) and rel_err(d0, dr0) < 1e-4
    synth.set_regime(n, "dense")
    n.set_blob("data", x); n.forward()
    d2, i2, R2 = n.detect(cap=8192, **kw)
    assert R2 == R and np.array_equal(i2, ids) and np.array_equal(d2, dets)
