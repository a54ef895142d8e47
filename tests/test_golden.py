"""Golden vectors produced by the reference's own layer sources (tests/golden/make_golden.py -> reference_layers.npz).
CPU: the oracle restatement reproduces them.  GPU (-m gpu): the HIP path reproduces them through the C ABI."""
import ast
import os

import numpy as np
import pytest

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_layers.npz"))
SHAPES = [(18, 60), (18, 60), (9, 30), (9, 30), (5, 15), (5, 15), (3, 8)]
FIELD = [60, 84, 120, 168, 240, 336, 480]; DS = [8, 8, 16, 16, 32, 32, 64]
BOX_CASES = ["dense", "sparse", "empty", "trunc", "norm"]
ROI_CASES = {"org": (7, 7, 0.125, 0.0), "ctx": (7, 7, 0.125, 0.25), "ped": (7, 5, 0.125, 0.25), "cal": (8, 4, 0.125, 0.0)}


def close(a, b, tol=1e-4):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    assert a.shape == b.shape
    assert (np.abs(a - b) / np.maximum(1, np.abs(b))).max() <= tol


# ---------------------------------------------------------------- CPU: oracle vs reference outputs
@pytest.mark.parametrize("case", BOX_CASES)
def test_oracle_boxoutput(orc, case):
    kw = ast.literal_eval(str(G[f"boxout_{case}_kw"]))
    rois, props, _, _ = orc.boxoutput([G[f"boxout_{case}_head{j}"] for j in range(7)], FIELD, FIELD, DS, **kw)
    assert np.array_equal(rois, G[f"boxout_{case}_rois"]) and np.array_equal(props, G[f"boxout_{case}_props"])


def test_oracle_roipool_decode_layers(orc):
    for tag, (ph, pw, sc, pad) in ROI_CASES.items():
        assert np.array_equal(orc.roipool(G["roipool_feat"], G["roipool_rois"], ph, pw, sc, pad), G[f"roipool_{tag}"])
    assert np.array_equal(orc.decode_bbox(G["decode_bbox"], G["decode_prior"], (0, 0, 0, 0), (0.1, 0.1, 0.2, 0.2)), G["decode_out"])
    close(orc.conv2d(G["conv_x"], G["conv_w"], G["conv_b"], (1, 1)), G["conv_y"])
    close(orc.conv2d(G["conv_x"], G["head_w"], G["conv_b"][:9], (3, 3)), G["head_y"])
    assert np.array_equal(orc.pool2d(G["conv_x"][:, :, :11, :19]), G["pool_y"])
    close(orc.inner_product(G["ip_x"], G["ip_w"], G["conv_b"][:10]), G["ip_y"])
    assert np.array_equal(orc.deconv2d(G["conv_x"], orc.bilinear_filler((16, 1, 4, 4)), None, (1, 1), (2, 2), 16), G["deconv_y"])


GB = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_layers_b.npz"))
ALIGN_CASES = {"a": (7, 7, 0.125, 0.0), "b": (7, 7, 0.125, 0.25), "c": (4, 6, 0.25, 0.5)}


def test_oracle_cascade_layers(orc):
    """ROIAlign, Eltwise, AVE pooling, Softmax of the cascade / WiderFace deploys against the reference's own outputs
    (tests/golden/make_golden_b.py)."""
    for tag, (ph, pw, sc, pad) in ALIGN_CASES.items():
        assert np.array_equal(orc.roialign(GB["roialign_feat"], GB["roialign_rois"], ph, pw, sc, pad), GB[f"roialign_{tag}"])
    xs = [GB["elt_a"], GB["elt_b"], GB["elt_c"]]
    assert np.array_equal(orc.eltwise(xs, "SUM"), GB["elt_sum"])
    close(orc.eltwise(xs[:2], "SUM", [0.5, 0.5]), GB["elt_avg"], 1e-6)     # reference: MKL saxpy (fma) -> 1 ulp
    assert np.array_equal(orc.eltwise(xs, "PROD"), GB["elt_prod"])
    assert np.array_equal(orc.eltwise(xs, "MAX"), GB["elt_max"])
    close(orc.pool2d(GB["ave_x"], (2, 2), (0, 0), (1, 1), "AVE"), GB["ave_y"], 1e-6)
    close(orc.softmax(GB["softmax_x"]), GB["softmax_y"], 1e-6)


# ---------------------------------------------------------------- GPU: HIP path vs reference outputs
@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X")
    from mscnn_amd import hipapi
    hipapi.lib()
    return hipapi


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("case", BOX_CASES)
def test_hip_boxoutput(hip, case):
    kw = ast.literal_eval(str(G[f"boxout_{case}_kw"]))
    d = hip.make_boxoutput_desc(SHAPES, 1, 9, FIELD, FIELD, DS, **kw)
    rois, props, aids, nreal = hip.BoxOutput(d).forward([dev(G[f"boxout_{case}_head{j}"]) for j in range(7)])
    assert np.array_equal(rois.cpu().numpy(), G[f"boxout_{case}_rois"])          # selection, order and boxes: bit-exact
    assert np.array_equal(props.cpu().numpy(), G[f"boxout_{case}_props"])


@pytest.mark.gpu
def test_hip_roipool_decode_layers(hip):
    for tag, (ph, pw, sc, pad) in ROI_CASES.items():
        y = hip.roipool(dev(G["roipool_feat"]), dev(G["roipool_rois"]), ph, pw, sc, pad)
        assert np.array_equal(y.cpu().numpy(), G[f"roipool_{tag}"])
    y = hip.decode_bbox(dev(G["decode_bbox"]), dev(G["decode_prior"]), (0, 0, 0, 0), (0.1, 0.1, 0.2, 0.2))
    assert np.array_equal(y.cpu().numpy(), G["decode_out"])
    close(hip.conv2d(dev(G["conv_x"]), dev(G["conv_w"]), dev(G["conv_b"]), (1, 1)).cpu().numpy(), G["conv_y"])
    close(hip.conv2d(dev(G["conv_x"]), dev(G["head_w"]), dev(G["conv_b"][:9]), (3, 3)).cpu().numpy(), G["head_y"])
    assert np.array_equal(hip.pool2d(dev(G["conv_x"][:, :, :11, :19])).cpu().numpy(), G["pool_y"])
    close(hip.inner_product(dev(G["ip_x"]), dev(G["ip_w"]), dev(G["conv_b"][:10])).cpu().numpy(), G["ip_y"])
    w = np.tile(np.outer([0.25, 0.75, 0.75, 0.25], [0.25, 0.75, 0.75, 0.25]).astype(np.float32), (16, 1, 1, 1))
    close(hip.deconv_depthwise(dev(G["conv_x"]), dev(w), None, (1, 1), (2, 2)).cpu().numpy(), G["deconv_y"], 1e-6)


@pytest.mark.gpu
def test_hip_cascade_layers(hip):
    for tag, (ph, pw, sc, pad) in ALIGN_CASES.items():
        y = hip.roialign(dev(GB["roialign_feat"]), dev(GB["roialign_rois"]), ph, pw, sc, pad)
        assert np.array_equal(y.cpu().numpy(), GB[f"roialign_{tag}"])
    xs = [dev(GB["elt_a"]), dev(GB["elt_b"]), dev(GB["elt_c"])]
    assert np.array_equal(hip.eltwise(xs, "SUM").cpu().numpy(), GB["elt_sum"])
    close(hip.eltwise(xs[:2], "SUM", [0.5, 0.5]).cpu().numpy(), GB["elt_avg"], 1e-6)
    assert np.array_equal(hip.eltwise(xs, "PROD").cpu().numpy(), GB["elt_prod"])
    assert np.array_equal(hip.eltwise(xs, "MAX").cpu().numpy(), GB["elt_max"])
    close(hip.pool2d(dev(GB["ave_x"]), (2, 2), (0, 0), (1, 1), "AVE").cpu().numpy(), GB["ave_y"], 1e-6)
    close(hip.softmax(dev(GB["softmax_x"])).cpu().numpy(), GB["softmax_y"], 1e-6)


# ---------------------------------------------------------------- third file: the stock layers (tests/golden/make_golden_c.py)
import stock_cases as sc  # noqa: E402

GC = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_layers_c.npz"))


def _stock_layers_against_the_reference(ops, relu_x):
    """ops: oracle.pyoracle, or the HIP front-end wrapped to take and return numpy (same signatures)."""
    off = 0
    for H, W, kh, kw, ph, pw, sh, sw, mi, Ho, Wo in GC["pool_cases"].tolist():
        n = sc.POOL_PLANES[0] * sc.POOL_PLANES[1] * Ho * Wo
        want = GC["pool_y"][off:off + n].reshape(sc.POOL_PLANES + (Ho, Wo)); off += n
        y = ops.pool2d(sc.pool_input(H, W), (kh, kw), (ph, pw), (sh, sw), ("MAX", "AVE")[mi])
        case = (H, W, kh, kw, ph, pw, sh, sw, mi)
        assert y.shape == want.shape, case                                  # the shape rule first
        if mi == 0:
            assert np.array_equal(y, want), case
        else:
            assert np.array_equal(np.isnan(y), np.isnan(want)), case
            assert np.allclose(y, want, rtol=0, atol=1e-6, equal_nan=True), case
    assert off == GC["pool_y"].size
    for slope, want in zip(sc.RELU_SLOPES, GC["relu_y"]):
        n = relu_x.size                                                         # (the device's inputs are a prefix of the recorded ones)
        assert np.array_equal(sc.bits(ops.relu(relu_x, slope)), sc.bits(want[:n])), slope
    cases = sc.deconv_cases()
    for i in GC["deconv_index"].tolist():
        x, w, b, g = sc.deconv_inputs(cases[i], i)
        close(ops.deconv2d(x, w, b, cases[i][3], cases[i][2], g), GC[f"deconv_y{i}"], 1e-6 if cases[i][0] == "dw" else 1e-4)
    seen = 0
    for tag, x in sc.softmax_inputs():
        if f"softmax_{tag}" in GC.files:
            want = GC[f"softmax_{tag}"]; y = ops.softmax(x); seen += 1
            assert np.array_equal(np.isnan(y), np.isnan(want)), tag
            assert np.allclose(y, want, rtol=0, atol=1e-6, equal_nan=True), tag
    assert seen == 16
    xs = sc.eltwise_inputs(8)
    for op in ("PROD", "MAX", "SUM"):
        assert np.array_equal(ops.eltwise(xs, op), GC[f"elt8_{op}"]), op
    close(ops.eltwise(xs, "SUM", sc.ELTWISE_COEFFS[8]), GC["elt8_coeff"], 1e-6)          # reference: MKL saxpy (fma) -> 1 ulp
    return True


def test_oracle_stock_layers(orc):
    """Pooling where the both-pads shape rule or an empty AVE window matters, ReLU specials (denormals included), one transposed
    convolution per family, Softmax with special rows, Eltwise with 8 bottoms, Concat: the oracle against the reference's outputs."""
    assert _stock_layers_against_the_reference(orc, sc.RELU_SPECIALS)
    for j, (axis, arrs) in enumerate(sc.concat_cases()):
        assert np.array_equal(orc.concat(arrs, axis), GC[f"concat_{j}"])


class _HipOps:
    """The HIP front-end behind the oracle's numpy signatures."""
    def __init__(self, hip):
        self.hip = hip

    def pool2d(self, x, k, p, s, m):
        return self.hip.pool2d(dev(x), k, p, s, m).cpu().numpy()

    def relu(self, x, slope):
        return self.hip.relu(dev(x), slope).cpu().numpy()

    def deconv2d(self, x, w, b, pad, stride, group):
        return self.hip.deconv2d(dev(x), dev(w), None if b is None else dev(b), pad, stride, group).cpu().numpy()

    def softmax(self, x):
        return self.hip.softmax(dev(x)).cpu().numpy()

    def eltwise(self, xs, op, coeffs=None):
        return self.hip.eltwise([dev(x) for x in xs], op, coeffs).cpu().numpy()


@pytest.mark.gpu
def test_hip_stock_layers(hip):
    """The same file through the C ABI (ReLU on +-0, +-inf and NaN: what the device does with denormals is not measured)."""
    assert _stock_layers_against_the_reference(_HipOps(hip), sc.RELU_SPECIALS_DEVICE)
    for j, (axis, arrs) in enumerate(sc.concat_cases()):
        if axis == 1:
            assert np.array_equal(hip.concat_channels([dev(a) for a in arrs]).cpu().numpy(), GC[f"concat_{j}"])


# ---------------------------------------------------------------- fourth file: the ROI layers and DecodeBBox (tests/golden/make_golden_d.py)
import roi_cases as rc  # noqa: E402

GD = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_layers_d.npz"))


def test_oracle_roi_layers_and_decode(orc):
    """ROIPooling / ROIAlign on both sides of the row kernel's limit, on maps with plateaus, NaN, +-inf and signed zeros, over ROIs that
    leave the map, are inverted or land on .5; DecodeBBox at every parameter set with overflowing, NaN and inf rows: the oracle
    against the reference's outputs, bit for bit (a NaN by position), and the reference's refusals of std <= 0 / NaN."""
    cases = rc.golden_d_cases()
    assert len(cases) == 20 and all(k in GD.files for k, *_ in cases)
    for key, op, kind, PH, PW, scale, pad in cases:
        feat = rc.feature_map(kind, rc.std_shape(rc.SWEEP_C))
        y = getattr(orc, op)(feat, rc.golden_d_rois(scale), PH, PW, scale, pad)
        assert y.shape == GD[key].shape, key
        assert np.array_equal(np.isnan(y), np.isnan(GD[key])) and np.array_equal(rc.bits(y), rc.bits(GD[key])), key
    assert any(np.isnan(GD[k]).any() for k, *_ in cases) and any(np.isinf(GD[k]).any() for k, *_ in cases)
    bbox, prior = rc.decode_inputs(257)
    for name, (mean, std) in rc.DECODE_PARAMS.items():
        y, want = orc.decode_bbox(bbox, prior, mean, std), GD[f"decode_{name}"]
        assert np.array_equal(np.isnan(y), np.isnan(want)) and np.array_equal(rc.bits(y), rc.bits(want)), name
    assert GD["decode_refused"].tolist() == [1] * len(rc.DECODE_REFUSED_STD)
    for std in rc.DECODE_REFUSED_STD:
        with pytest.raises(ValueError, match=r"bbox_std\[\d\]"):
            orc.decode_bbox(bbox, prior, (0, 0, 0, 0), std)


@pytest.mark.gpu
def test_hip_roi_layers_and_decode(hip):
    """The same file through the C ABI.  Plain and post-ReLU maps bit for bit; on the special map NaN positions, values under == and
    the bits of every non-zero value (the sign of a zero of a -0 / +0 tie is the row kernel's to choose).  DecodeBBox rows whose
    exponents lie inside expf_libm's table range (-87, 87) bit for bit."""
    for key, op, kind, PH, PW, scale, pad in rc.golden_d_cases():
        feat = rc.feature_map(kind, rc.std_shape(rc.SWEEP_C))
        y = getattr(hip, op)(dev(feat), dev(rc.golden_d_rois(scale)), PH, PW, scale, pad).cpu().numpy()
        want = GD[key]
        assert y.shape == want.shape and np.array_equal(np.isnan(y), np.isnan(want)), key
        ok = ~np.isnan(want)
        assert np.array_equal(y[ok], want[ok]), key
        nz = ok & (want != 0) if kind == "special" else ok
        assert np.array_equal(y[nz].view(np.uint32), want[nz].view(np.uint32)), key
    bbox, prior = rc.decode_inputs(257)
    for name, (mean, std) in rc.DECODE_PARAMS.items():
        y, want = hip.decode_bbox(dev(bbox), dev(prior), mean, std).cpu().numpy(), GD[f"decode_{name}"]
        e = bbox[:, 6:8] * np.array(std[2:], np.float32) + np.array(mean[2:], np.float32)
        inside = (np.abs(e) < 87).all(1) & np.isfinite(bbox[:, 4:]).all(1)
        assert inside.sum() > 200 and np.array_equal(rc.bits(y[inside]), rc.bits(want[inside])), name
