"""Pins the C restatement (oracle/mscnn_oracle.c) to the reference's OWN sources compiled by oracle/ref.mk
(oracle/_ref/libmscnn_ref.so).  CPU only; skipped where _ref has not been built (it needs the reference checkout)."""
import numpy as np
import pytest

from oracle import pyref

pytestmark = pytest.mark.skipif(not pyref.available(), reason="oracle/_ref not built (needs /root/reference at build time)")


def _rois(rng, R, H, W, batch=1):
    x1 = rng.uniform(-60, W, R); y1 = rng.uniform(-60, H, R)
    return np.stack([rng.integers(0, batch, R), x1, y1, x1 + rng.uniform(0, 600, R), y1 + rng.uniform(0, 400, R)], 1).astype(np.float32)


@pytest.mark.parametrize("cfg", [
    (1, 16, 20, 30, 8, (3, 3), (1, 1), (1, 1), 1), (2, 6, 9, 7, 4, (3, 3), (0, 0), (2, 2), 2),
    (1, 32, 18, 60, 9, (5, 5), (2, 2), (1, 1), 1), (1, 8, 12, 20, 7, (7, 5), (3, 2), (1, 1), 1), (3, 16, 7, 7, 12, (3, 3), (0, 0), (1, 1), 1),
])
def test_conv(orc, cfg):
    N, Cin, H, W, Cout, k, pad, stride, g = cfg
    rng = np.random.default_rng(1)
    x = rng.standard_normal((N, Cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin // g, *k)) * 0.1).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32)
    a, r = orc.conv2d(x, w, b, pad, stride, g), pyref.conv2d(x, w, b, pad, stride, g)
    assert a.shape == r.shape
    assert np.abs(a - r).max() <= 1e-4 * max(1.0, np.abs(r).max())      # BLAS summation order is unspecified


def test_pool_relu_softmax_ip_deconv(orc):
    rng = np.random.default_rng(2)
    x = rng.standard_normal((2, 5, 15, 21)).astype(np.float32)
    for k, p, s, m in [((2, 2), (0, 0), (2, 2), "MAX"), ((3, 3), (1, 1), (2, 2), "MAX"), ((2, 2), (0, 0), (1, 1), "AVE"), ((3, 3), (1, 1), (2, 2), "AVE")]:
        a, r = orc.pool2d(x, k, p, s, m), pyref.pool2d(x, k, p, s, m)
        assert a.shape == r.shape and (np.array_equal(a, r) if m == "MAX" else np.allclose(a, r, atol=1e-6))
    assert np.array_equal(orc.relu(x), pyref.relu(x))
    assert np.allclose(orc.relu(x, 0.1), pyref.relu(x, 0.1), atol=1e-7)
    xi = rng.standard_normal((6, 5)).astype(np.float32)
    assert np.allclose(orc.softmax(xi), pyref.softmax(xi), atol=1e-7)
    w = rng.standard_normal((11, 5 * 15 * 21)).astype(np.float32) * 0.05; b = rng.standard_normal(11).astype(np.float32)
    assert np.allclose(orc.inner_product(x, w, b), pyref.inner_product(x, w, b), atol=1e-4)
    xd = rng.standard_normal((1, 6, 7, 9)).astype(np.float32)
    wd = rng.standard_normal((6, 1, 4, 4)).astype(np.float32)
    assert np.allclose(orc.deconv2d(xd, wd, None, (1, 1), (2, 2), 6), pyref.deconv2d(xd, wd, None, (1, 1), (2, 2), 6), atol=1e-6)
    assert np.array_equal(orc.deconv2d(xd, orc.bilinear_filler((6, 1, 4, 4)), None, (1, 1), (2, 2), 6),
                          pyref.deconv2d(xd, None, None, (1, 1), (2, 2), 6, kernel=(4, 4), num_output=6, bilinear=True))
    wg = rng.standard_normal((6, 2, 3, 3)).astype(np.float32)     # generic (non-depthwise) transposed conv, groups
    assert np.allclose(orc.deconv2d(xd, wg, None, (0, 0), (2, 2), 2), pyref.deconv2d(xd, wg, None, (0, 0), (2, 2), 2), atol=1e-5)


@pytest.mark.parametrize("ph,pw,scale,pad", [(7, 7, 0.125, 0.0), (7, 7, 0.125, 0.25), (7, 5, 0.25, 0.25), (8, 4, 0.125, 0.0), (3, 3, 1.0, 0.5)])
def test_roipool_bitexact(orc, ph, pw, scale, pad):
    rng = np.random.default_rng(3)
    feat = rng.standard_normal((2, 7, 36, 120)).astype(np.float32)
    rois = _rois(rng, 200, 36 / scale, 120 / scale, 2)
    assert np.array_equal(orc.roipool(feat, rois, ph, pw, scale, pad), pyref.roipool(feat, rois, ph, pw, scale, pad))


@pytest.mark.parametrize("ph,pw,scale,pad", [(7, 7, 0.125, 0.0), (7, 7, 0.125, 0.25), (4, 4, 0.25, 0.5)])
def test_roialign_bitexact(orc, ph, pw, scale, pad):
    rng = np.random.default_rng(13)
    feat = rng.standard_normal((2, 5, 36, 120)).astype(np.float32)
    rois = _rois(rng, 150, 36 / scale, 120 / scale, 2)
    rois[:10, 3] = rois[:10, 1] - 5                     # malformed (negative width) -> zeros
    assert np.array_equal(orc.roialign(feat, rois, ph, pw, scale, pad), pyref.roialign(feat, rois, ph, pw, scale, pad))


def test_eltwise(orc):
    rng = np.random.default_rng(14)
    xs = [rng.standard_normal((7, 5)).astype(np.float32) for _ in range(3)]
    for op in ("PROD", "MAX"):
        assert np.array_equal(orc.eltwise(xs, op), pyref.eltwise(xs, op))
    assert np.array_equal(orc.eltwise(xs[:2], "MAX"), pyref.eltwise(xs[:2], "MAX"))
    assert np.allclose(orc.eltwise(xs, "SUM", [0.33333333] * 3), pyref.eltwise(xs, "SUM", [0.33333333] * 3), atol=1e-6)   # saxpy may fuse
    assert np.array_equal(orc.eltwise(xs, "SUM"), pyref.eltwise(xs, "SUM"))


def test_decode_bbox_bitexact(orc):
    rng = np.random.default_rng(4)
    prior = _rois(rng, 300, 576, 1920)
    bbox = (rng.standard_normal((300, 8)) * 2).astype(np.float32)
    for mean, std in [((0, 0, 0, 0), (1, 1, 1, 1)), ((0, 0, 0, 0), (0.1, 0.1, 0.2, 0.2)), ((0.1, -0.1, 0.05, 0), (0.2, 0.2, 0.3, 0.3))]:
        assert np.array_equal(orc.decode_bbox(bbox, prior, mean, std), pyref.decode_bbox(bbox, prior, mean, std))


def test_box_iou_bitexact(orc):
    rng = np.random.default_rng(5)
    for _ in range(2000):
        a = rng.uniform(0, 100, 4).astype(np.float32); b = (a + rng.normal(0, 10, 4)).astype(np.float32)
        for mode in ("IOU", "IOMU", "IOFU"):
            assert orc.box_iou(a, b, mode) == pyref.box_iou(a, b, mode)


SHAPES = [(18, 60), (18, 60), (9, 30), (9, 30), (5, 15), (5, 15), (3, 8)]
FIELD = [60, 84, 120, 168, 240, 336, 480]
DS = [8, 8, 16, 16, 32, 32, 64]


@pytest.mark.parametrize("bg,kw", [
    (-8.0, dict()), (4.0, dict()), (-8.0, dict(max_nms_num=100)), (-8.0, dict(max_post_nms_num=37)), (60.0, dict()),
    (-8.0, dict(nms_type="IOMU", iou_thr=0.5)), (-8.0, dict(nms_type="IOFU", iou_thr=0.7)),
    (-8.0, dict(bbox_mean=[0, 0, 0, 0], bbox_std=[0.1, 0.1, 0.2, 0.2], min_size=5.0)), (-2.0, dict(fg_thr=-7.0, field_whr=3.0, field_xyr=4.0)),
])
def test_boxoutput_bitexact(orc, bg, kw):
    rng = np.random.default_rng(6)
    heads = []
    for (h, w) in SHAPES:
        t = rng.standard_normal((2, 9, h, w)).astype(np.float32)
        t[:, :5] *= 2; t[:, 0] += bg; t[:, 5:] *= 0.5
        t[:, 1:3, :2, :] = 1.25                      # score plateaus: exact ties
        heads.append(t)
    a = orc.boxoutput(heads, FIELD, FIELD, DS, **kw)
    r = pyref.boxoutput(heads, FIELD, FIELD, DS, **kw)
    assert a[0].shape == r[0].shape
    assert np.array_equal(a[0], r[0]) and np.array_equal(a[1], r[1])


def test_small_net_end_to_end(orc):
    """The oracle net executor on both back-ends: same graph, restatement vs the reference's own layer classes."""
    from mscnn_amd import net as mnet, synth, zoo
    from oracle import pynet
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=128, width=256, max_nms_num=60), device=-1)
    layers = [(n.layer_names[i], n.layer_types[i], n.layer_bottoms(i), n.layer_tops(i), n.layer_param_text(i)) for i in range(len(n.layer_names))]
    ws = synth.weights(n.layer_names, n.layer_types, [n.param_shapes(i) for i in range(len(n.layer_names))], "mid")
    x = synth.frame(128, 256)
    a = pynet.forward(layers, ws, {"data": x})
    r = pynet.forward(layers, ws, {"data": x}, backend=pyref)
    for b in ("conv4_3", "conv6_1", "LFCN_1_7x7", "LFCN_4_5x5"):
        assert np.abs(a[b] - r[b]).max() <= 1e-4 * max(1.0, np.abs(r[b]).max()), b
    # same graph, same heads -> same proposals (feed the reference's heads to the restatement to avoid BLAS-order flips)
    bo = [l for l in layers if l[1] == "BoxOutput"][0]
    a2 = pynet.forward([bo], ws, {k: r[k] for k in bo[2]})
    assert np.array_equal(a2["proposals"], r["proposals"]) and np.array_equal(a2["proposals_score"], r["proposals_score"])


# ---------------------------------------------------------------- the stock layers over their whole parameter space
import stock_cases as sc  # noqa: E402


def test_pool_sweep_shape_rule_and_values(orc):
    """Every kernel / pad < kernel / stride in {1,2,3} per dimension on 20 map sizes, MAX and AVE (12 960 combinations): the
    output SHAPE first (the reference clips the last window of both dimensions when either pad is non-zero), MAX bit for bit,
    AVE within 1e-6 with identical NaN positions (0 / 0 of a window that lies wholly past the map).  What the reference's
    set-up refuses, the oracle refuses."""
    total = refused = nan_cases = 0
    for H, W in sc.POOL_SIZES:
        x = sc.pool_input(H, W)
        for k, p, s in sc.pool_params():
            for m in ("MAX", "AVE"):
                total += 1
                try:
                    r = pyref.pool2d(x, k, p, s, m)
                except RuntimeError:
                    refused += 1
                    with pytest.raises(ValueError):
                        orc.pool2d(x, k, p, s, m)
                    continue
                assert orc.pool_out_dims(H, W, k, p, s) == r.shape[2:], (H, W, k, p, s)
                a = orc.pool2d(x, k, p, s, m)
                assert a.shape == r.shape, (H, W, k, p, s, m)
                if m == "MAX":
                    assert np.array_equal(a, r), (H, W, k, p, s)
                else:
                    assert np.array_equal(np.isnan(a), np.isnan(r)), (H, W, k, p, s)
                    assert np.allclose(a, r, rtol=0, atol=1e-6, equal_nan=True), (H, W, k, p, s)
                    nan_cases += bool(np.isnan(r).any())
    print(f"pool sweep: {total} combinations, {refused} refused by the reference, {nan_cases} AVE cases with NaN")
    assert total == 12960 and nan_cases > 0


def test_pool_refusals_match(orc):
    """Outside the sweep (pad >= kernel, a kernel larger than the padded map): refused on both sides."""
    x = sc.pool_input(3, 4)
    for k, p, s in [((2, 2), (2, 0), (1, 1)), ((1, 3), (0, 3), (2, 2)), ((3, 3), (1, 4), (1, 1)), ((5, 2), (0, 0), (1, 1))]:
        with pytest.raises(RuntimeError):
            pyref.pool2d(x, k, p, s, "MAX")
        with pytest.raises(ValueError):
            orc.pool2d(x, k, p, s, "MAX")


def test_relu_special_values_bit_patterns(orc):
    for slope in sc.RELU_SLOPES:
        a, r = orc.relu(sc.RELU_SPECIALS, slope), pyref.relu(sc.RELU_SPECIALS, slope)
        assert np.array_equal(np.isnan(a), np.isnan(r)), slope
        assert np.array_equal(sc.bits(a), sc.bits(r)), (slope, a, r)
    x = np.random.default_rng(21).standard_normal(4099).astype(np.float32)
    for slope in sc.RELU_SLOPES:
        assert np.array_equal(sc.bits(orc.relu(x, slope)), sc.bits(pyref.relu(x, slope)))


def test_softmax_shapes_scales_specials(orc):
    for tag, x in sc.softmax_inputs():
        a, r = orc.softmax(x), pyref.softmax(x)
        assert np.array_equal(np.isnan(a), np.isnan(r)), tag
        assert np.allclose(a, r, rtol=0, atol=1e-6, equal_nan=True), tag
        if not tag.endswith(("x1", "x30", "x100", "pm1000")):
            assert np.isnan(r).any(), tag                   # the special row is NaN in the reference (inf - inf)


def test_deconv_generic_and_depthwise(orc):
    for i, case in enumerate(sc.deconv_cases()):
        x, w, b, g = sc.deconv_inputs(case, i)
        a, r = orc.deconv2d(x, w, b, case[3], case[2], g), pyref.deconv2d(x, w, b, case[3], case[2], g)
        assert a.shape == r.shape, case
        assert np.allclose(a, r, atol=1e-6 if case[0] == "dw" else 1e-5), case


def test_eltwise_bottom_counts(orc):
    for nb in sc.ELTWISE_BOTTOMS:
        xs = sc.eltwise_inputs(nb)
        for op in ("PROD", "MAX", "SUM"):
            assert np.array_equal(orc.eltwise(xs, op), pyref.eltwise(xs, op)), (nb, op)
        cf = sc.ELTWISE_COEFFS[nb]
        assert min(cf) < 0 and 0.0 in cf
        assert np.allclose(orc.eltwise(xs, "SUM", cf), pyref.eltwise(xs, "SUM", cf), atol=1e-6), nb      # saxpy may fuse
        assert (np.stack(xs).max(0) == xs[0]).reshape(-1)[::3].any()                                       # a tie wins somewhere


@pytest.mark.skipif(not pyref.has("ref_concat"), reason="oracle/_ref predates ref_concat and was not rebuilt (make -C oracle ref needs the reference checkout)")
def test_concat_axes(orc):
    for axis, xs in sc.concat_cases():
        assert np.array_equal(orc.concat(xs, axis), pyref.concat(xs, axis)), (axis, xs[0].shape)


# ---------------------------------------------------------------- the ROI layers and DecodeBBox over their parameter space
import roi_cases as rc  # noqa: E402


def _same_but_nan_payloads(a, r, what):
    """Bit for bit; a NaN is compared by position only."""
    assert a.shape == r.shape, what
    assert np.array_equal(np.isnan(a), np.isnan(r)), what
    assert np.array_equal(rc.bits(a), rc.bits(r)), what


@pytest.mark.parametrize("kind", rc.MAP_KINDS)
@pytest.mark.parametrize("op", ["roipool", "roialign"])
def test_roi_layers_sweep(orc, op, kind):
    """ROIPooling / ROIAlign at every pooled size of roi_cases.sweep_sizes() (heights and widths 1 .. 20, 15 | 16 | 17 both ways), scales
    1/16 .. 1, pads 0 .. 1, on the plain, the post-ReLU and the special map (NaN, +-inf, -FLT_MAX-scale, signed zeros), over the hand
    rows (outside on every side, inverted, .5 edges, single point, whole map) and random ROIs."""
    feat = rc.feature_map(kind, rc.std_shape(rc.SWEEP_C))
    n = 0
    for scale in rc.SWEEP_SCALES:
        rois = rc.std_rois(*rc.STD_HW, 2, scale, n_random=25)
        for pad in rc.SWEEP_PADS:
            for PH, PW in rc.sweep_sizes():
                a, r = getattr(orc, op)(feat, rois, PH, PW, scale, pad), getattr(pyref, op)(feat, rois, PH, PW, scale, pad)
                _same_but_nan_payloads(a, r, (op, kind, PH, PW, scale, pad))
                n += 1
    print(f"{op} on {kind}: {n} combinations x {len(rois)} ROIs")
    assert n == 25 * len(rc.sweep_sizes())


def test_roipool_wide_and_tall_maps(orc):
    """The maps of the row kernel's segment and row-tail cases: the oracle the GPU tests compare with, held to the reference there too."""
    for tag, mk, rois, PH, PW, scale, pad in rc.row_cases():
        if mk != "std":
            for kind in rc.MAP_KINDS:
                feat = rc.feature_map(kind, rc.case_shape(mk, 8))
                _same_but_nan_payloads(orc.roipool(feat, rois, PH, PW, scale, pad), pyref.roipool(feat, rois, PH, PW, scale, pad), (tag, kind))


def test_decode_bbox_sweep(orc):
    """The zoo's three std sets, identity and a non-zero mean, at R = 1 .. 257 with exponents across (-104, 100), NaN / inf rows and
    inverted priors; the dense exponent sweep over (-87, 87) and the rows beyond it."""
    for R in rc.DECODE_ROWS:
        bbox, prior = rc.decode_inputs(R)
        for name, (mean, std) in rc.DECODE_PARAMS.items():
            _same_but_nan_payloads(orc.decode_bbox(bbox, prior, mean, std), pyref.decode_bbox(bbox, prior, mean, std), (R, name))
    for bbox, prior in (rc.decode_sweep(1 << 15)[:2], rc.decode_beyond()):
        bbox, prior = bbox[:1 << 16], prior[:1 << 16]
        _same_but_nan_payloads(orc.decode_bbox(bbox, prior), pyref.decode_bbox(bbox, prior), len(bbox))


@pytest.mark.parametrize("std", rc.DECODE_REFUSED_STD)
def test_decode_bbox_refusals_match(orc, std):
    """std <= 0, -0 and NaN: refused by the reference's set-up (decode_bbox_layer.cpp:30), so refused by the oracle, naming the value."""
    bbox, prior = rc.decode_inputs(4)
    with pytest.raises(RuntimeError):
        pyref.decode_bbox(bbox, prior, (0, 0, 0, 0), std)
    with pytest.raises(ValueError, match=r"bbox_std\[\d\] = \S+ must be > 0"):
        orc.decode_bbox(bbox, prior, (0, 0, 0, 0), std)
