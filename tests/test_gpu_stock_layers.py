"""The stock layers of mscnn_amd/csrc/elementwise.hip over their parameter space and through every branch of their kernels: the
pooling sweep against the oracle that tests/test_oracle_vs_ref.py pins to the reference, the fast 2x2 pooling kernel against the
general one on the same data, the second trip of every grid-stride loop (grids are capped at 2048 workgroups of 256 threads, so
the second trip starts at work item 524 288), the depthwise transposed convolution's quad kernel past its first x-block and its
N * C > 65535 fallback, the generic transposed convolution, ReLU on special values, Softmax, Eltwise and the Pooling host layer.
Bars: MAX / selection bit-exact, AVE / Softmax / depthwise within 1e-6, generic transposed convolution 1e-4 relative."""
import numpy as np
import pytest

import stock_cases as sc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TRIP = 2048 * 256          # work items of one trip of a grid-stride loop (kMaxBlocks * kThreads)


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X: torch.cuda.is_available() is False")
    from mscnn_amd import hipapi
    hipapi.lib()
    return hipapi


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def close(a, b, tol=1e-4):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    assert err.max() <= tol, f"max rel err {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}"


def shifted_empty(shape):
    """A contiguous tensor whose base lies one float into a larger allocation: 4-byte aligned and no better, so every kernel
    that needs 8 or 16 bytes gives way to its general form."""
    n = int(np.prod(shape))
    v = torch.empty(n + 1, dtype=torch.float32, device="cuda")[1:].view(*shape)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def shifted(a):
    v = shifted_empty(a.shape)
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return v


def pool_into(hip, x, y, k=(2, 2), p=(0, 0), s=(2, 2), m="MAX"):
    N, Cc, H, W = x.shape
    assert tuple(y.shape) == (N, Cc) + hip.pool_out_dims(H, W, k, p, s)
    hip._check(hip.lib().mscnn_pool2d_fwd_f32(hip._dev(x), hip._dev(y), N, Cc, H, W, k[0], k[1], p[0], p[1], s[0], s[1], 0 if m == "MAX" else 1,
                                              hip._stream()))
    return y


def deconv_dw_into(hip, x, w, b, y, pad, stride):
    N, Cc, H, W = x.shape
    hip._check(hip.lib().mscnn_deconv_depthwise_fwd_f32(hip._dev(x), hip._dev(w), hip._dev(b), hip._dev(y), N, Cc, H, W, w.shape[2], w.shape[3],
                                                        pad[0], pad[1], stride[0], stride[1], hip._stream()))
    return y


def check_ave(y, ref, what):
    assert y.shape == ref.shape, what
    assert np.array_equal(np.isnan(y), np.isnan(ref)), what
    assert np.allclose(y, ref, rtol=0, atol=1e-6, equal_nan=True), what


# ------------------------------------------------------------------------------------------------ pooling
def test_pool_sweep_against_the_pinned_oracle(hip, orc):
    """Every kernel, pad < kernel and stride in {1,2,3} per dimension, MAX and AVE, on a 3x4 and a 7x8 map: the shape is the
    reference's rule (either pad clips both dimensions), MAX bit for bit, AVE within 1e-6 with the NaNs of the empty windows
    (0 / 0) where the oracle has them."""
    nan_cases = clipped = 0
    for H, W in sc.POOL_SIZES_GPU:
        x = sc.pool_input(H, W); xd = dev(x)
        for k, p, s in sc.pool_params():
            dims = orc.pool_out_dims(H, W, k, p, s)
            assert hip.pool_out_dims(H, W, k, p, s) == dims, (H, W, k, p, s)
            clipped += dims != sc.pool_dims_per_dimension(H, W, k, p, s)
            for m in ("MAX", "AVE"):
                y = hip.pool2d(xd, k, p, s, m).cpu().numpy()
                ref = orc.pool2d(x, k, p, s, m)
                assert y.shape == ref.shape == x.shape[:2] + dims
                if m == "MAX":
                    assert np.array_equal(y, ref), (H, W, k, p, s)
                else:
                    check_ave(y, ref, (H, W, k, p, s))
                    nan_cases += bool(np.isnan(ref).any())
    assert nan_cases > 0 and clipped > 0          # the sweep holds what it is for
    y = hip.pool2d(dev(sc.pool_input(3, 4)), (1, 2), (0, 1), (3, 1), "MAX")          # the smallest case the old per-dimension rule got wrong
    assert tuple(y.shape[2:]) == (1, 5)
    for k, p in (((2, 2), (2, 0)), ((1, 3), (0, 3)), ((5, 2), (0, 0))):               # refused by the reference's set-up: an error, no launch
        with pytest.raises(hip.MscnnError):
            hip.pool2d(dev(sc.pool_input(3, 4)), k, p, (1, 1), "MAX")


@pytest.mark.parametrize("shape", [(2, 3, 8, 12), (1, 2, 64, 260)])
def test_pool_fast_kernel_is_bit_identical_to_the_general_kernel(hip, orc, shape):
    """2x2 / stride 2 MAX: maxpool2x2_kernel (x 16-byte, y 8-byte aligned) against pool_general_kernel, reached with x -- and then
    y -- one float into a larger buffer.  Values repeat (ties) and the first-max-wins order must not show."""
    rng = np.random.default_rng(31)
    x = rng.integers(-3, 4, shape).astype(np.float32) + rng.integers(0, 2, shape).astype(np.float32) * 0.5
    fast = hip.pool2d(dev(x)).cpu().numpy()
    gen_x = hip.pool2d(shifted(x)).cpu().numpy()
    gen_y = pool_into(hip, dev(x), shifted_empty(fast.shape)).cpu().numpy()
    assert fast.tobytes() == gen_x.tobytes() == gen_y.tobytes()
    assert np.array_equal(fast, orc.pool2d(x))


@pytest.mark.parametrize("shape", [(1, 2, 9, 12), (1, 2, 8, 6), (1, 2, 8, 10), (1, 2, 9, 10)])
def test_pool_shapes_next_to_the_fast_path_take_the_general_kernel(hip, orc, shape):
    """H odd (the last row is half a window) or W % 4 == 2: not the fast kernel's shapes; ceil-mode edges against the oracle."""
    x = np.random.default_rng(32).standard_normal(shape).astype(np.float32)
    y = hip.pool2d(dev(x)).cpu().numpy()
    assert y.shape[2:] == ((shape[2] + 1) // 2, (shape[3] + 1) // 2)
    assert np.array_equal(y, orc.pool2d(x))


# ------------------------------------------------------------------------------------------------ second trip of the grid-stride loops
def test_second_trip_relu_both_kernels(hip, orc):
    rng = np.random.default_rng(41)
    for n, kernel in ((4 * TRIP + 4, "float4"), (TRIP + 3, "scalar")):
        x = rng.standard_normal(n).astype(np.float32)
        assert np.array_equal(sc.bits(hip.relu(dev(x)).cpu().numpy()), sc.bits(orc.relu(x))), kernel
        close(hip.relu(dev(x), 0.1).cpu().numpy(), orc.relu(x, 0.1), 1e-6)


def test_second_trip_eltwise(hip, orc):
    rng = np.random.default_rng(42)
    n = TRIP + 5
    xs = [rng.standard_normal(n).astype(np.float32) for _ in range(8)]
    xs[1][::3] = xs[0][::3]; xs[2][-5:] = xs[0][-5:] + 1          # ties, and the tail decided by the last of three bottoms
    ds = [dev(x) for x in xs]
    for op, cf in (("PROD", None), ("SUM", None), ("MAX", None), ("SUM", sc.ELTWISE_COEFFS[3])):
        assert np.array_equal(hip.eltwise(ds[:3], op, cf).cpu().numpy(), orc.eltwise(xs[:3], op, cf)), op
    assert np.array_equal(hip.eltwise(ds, "SUM", sc.ELTWISE_COEFFS[8]).cpu().numpy(), orc.eltwise(xs, "SUM", sc.ELTWISE_COEFFS[8]))


def test_second_trip_concat_into_a_channel_window(hip):
    """Per-image size 3, N = 174 763 (524 289 elements), written at channel offset 1 of a 5-channel blob: the window holds x, every
    byte outside it is unchanged."""
    N, Cc, ctot, off = 174763, 3, 5, 1
    assert N * Cc == TRIP + 1
    x = np.random.default_rng(43).standard_normal((N, Cc, 1, 1)).astype(np.float32)
    y = torch.full((N, ctot, 1, 1), -7.25, dtype=torch.float32, device="cuda")
    hip._check(hip.lib().mscnn_concat_channels_f32(hip._dev(dev(x)), hip._dev(y), N, Cc, 1, ctot, off, hip._stream()))
    y = y.cpu().numpy()
    assert np.array_equal(y[:, off:off + Cc], x)
    assert (y[:, :off] == -7.25).all() and (y[:, off + Cc:] == -7.25).all()


def test_second_trip_softmax(hip, orc):
    outer, Cc, inner = (TRIP + 7) // 3, 2, 3
    assert outer * inner == TRIP + 7
    x = (np.random.default_rng(44).standard_normal((outer, Cc, inner)) * 3).astype(np.float32)
    y = hip.softmax(dev(x)).cpu().numpy()
    close(y, orc.softmax(x), 1e-6)
    assert np.abs(y.astype(np.float64).sum(1) - 1).max() <= 1e-6


def test_second_trip_pooling(hip, orc):
    """pool_general_kernel, AVE 3x3 / stride 1 on (1, 33, 128, 128): 523 908 outputs without a pad (one trip, 380 short of the
    second) and 540 672 with pad 1 (the second trip); maxpool2x2_kernel on (1, 65, 256, 256): 532 480 work items."""
    rng = np.random.default_rng(45)
    x = rng.standard_normal((1, 33, 128, 128)).astype(np.float32)
    for pad in ((0, 0), (1, 1)):
        close(hip.pool2d(dev(x), (3, 3), pad, (1, 1), "AVE").cpu().numpy(), orc.pool2d(x, (3, 3), pad, (1, 1), "AVE"), 1e-6)
    assert 33 * 126 * 126 < TRIP < 33 * 128 * 128
    assert np.array_equal(hip.pool2d(dev(x), (3, 3), (1, 1), (1, 1), "MAX").cpu().numpy(), orc.pool2d(x, (3, 3), (1, 1), (1, 1), "MAX"))
    x = rng.standard_normal((1, 65, 256, 256)).astype(np.float32)
    assert 65 * 128 * 64 > TRIP
    assert np.array_equal(hip.pool2d(dev(x)).cpu().numpy(), orc.pool2d(x))


def test_second_trip_transposed_convolutions(hip, orc):
    rng = np.random.default_rng(46)
    x = rng.standard_normal((1, 9, 128, 128)).astype(np.float32)                # deconv_dw_kernel: 2x2 / stride 2 -> 589 824 outputs
    w = rng.standard_normal((9, 1, 2, 2)).astype(np.float32); b = rng.standard_normal(9).astype(np.float32)
    close(hip.deconv_depthwise(dev(x), dev(w), dev(b), (0, 0), (2, 2)).cpu().numpy(), orc.deconv2d(x, w, b, (0, 0), (2, 2), group=9), 1e-6)
    x = rng.standard_normal((1, 4, 64, 96)).astype(np.float32)                  # deconv_generic_kernel: 24 x 129 x 193 = 597 528 outputs
    w = (rng.standard_normal((4, 12, 3, 3)) * 0.5).astype(np.float32); b = rng.standard_normal(24).astype(np.float32)
    y = hip.deconv2d(dev(x), dev(w), dev(b), (0, 0), (2, 2), 2).cpu().numpy()
    assert y.shape == (1, 24, 129, 193) and y.size > TRIP
    close(y, orc.deconv2d(x, w, b, (0, 0), (2, 2), group=2))


def test_second_trip_metric_kernels(hip):
    """sum_squares, max_rel_diff and max_rel_diff_strided on 524 288 + 300 floats with the deciding element among the last 300;
    then a NaN there (+inf from the two difference kernels, NaN from the sum), then the NaN one float past the compared range
    (not seen)."""
    n = TRIP + 300
    rng = np.random.default_rng(47)
    ref = (rng.standard_normal(n + 1) * 7).astype(np.float32)
    a = (ref + rng.standard_normal(n + 1).astype(np.float32) * 1e-3).astype(np.float32)
    ref[n - 5] = 0.5; a[n - 5] = 40.5                  # the maximum, in the tail
    ref[n - 9] = 3000.0; a[n - 9] = 3000.0            # ... and most of the sum of squares
    f64 = lambda t: float(t.cpu()[0])                  # noqa: E731
    want_ss = float((ref[:n].astype(np.float64) ** 2).sum())
    assert ref[n - 9].astype(np.float64) ** 2 > 0.2 * want_ss
    assert abs(f64(hip.sum_squares(dev(ref)[:n])) - want_ss) <= 1e-9 * want_ss
    want = (np.abs(a[:n].astype(np.float64) - ref[:n]) / np.maximum(1.0, np.abs(ref[:n]))).max()
    assert want > 1.0 and abs(f64(hip.max_rel_diff(dev(a)[:n], dev(ref)[:n])) - want) <= 1e-6 * want
    # strided: 4 planes of `run` floats, plane strides run + 3 (a) and run + 1 (ref): gaps between the runs and behind the last
    planes, run = 4, n // 4
    assert planes * run == n
    sa, sr = run + 3, run + 1
    A = np.full(planes * sa, 1e9, np.float32); R = np.full(planes * sr, -1e9, np.float32)
    for p in range(planes):
        A[p * sa:p * sa + run] = a[p * run:(p + 1) * run]; R[p * sr:p * sr + run] = ref[p * run:(p + 1) * run]
    ss = hip.sum_squares(dev(ref)[:n])
    floor = max(1.0, np.sqrt(want_ss / n))
    want_s = (np.abs(a[:n].astype(np.float64) - ref[:n]) / np.maximum(floor, np.abs(ref[:n]))).max()
    strided = lambda Ad: f64(hip.max_rel_diff_strided(Ad, sa, dev(R), sr, planes, run, ss, n))      # noqa: E731
    assert abs(strided(dev(A)) - want_s) <= 1e-5 * want_s
    # a NaN in the tail
    bad = a.copy(); bad[n - 2] = np.nan
    assert np.isposinf(f64(hip.max_rel_diff(dev(bad)[:n], dev(ref)[:n])))
    assert np.isnan(f64(hip.sum_squares(dev(bad)[:n])))
    Ab = A.copy(); Ab[3 * sa + run - 2] = np.nan
    assert np.isposinf(strided(dev(Ab)))
    # a NaN one float past the range
    bad = a.copy(); bad[n] = np.nan
    assert abs(f64(hip.max_rel_diff(dev(bad)[:n], dev(ref)[:n])) - want) <= 1e-6 * want
    assert abs(f64(hip.sum_squares(dev(bad)[:n])) - float((a[:n].astype(np.float64) ** 2).sum())) <= 1e-9 * want_ss
    Ab = A.copy(); Ab[3 * sa + run] = np.nan; Ab[run] = np.nan
    assert abs(strided(dev(Ab)) - want_s) <= 1e-5 * want_s


# ------------------------------------------------------------------------------------------------ transposed convolution
@pytest.mark.parametrize("shape,bias", [((1, 2, 3, 257), True), ((2, 3, 2, 300), False), ((1, 2, 1, 5), True), ((1, 2, 4, 1), False),
                                        ((1, 1, 3, 7), True), ((1, 1, 1, 1), True)])
def test_deconv_quad_kernel_is_bit_identical_to_the_per_output_kernel(hip, orc, shape, bias):
    """4x4 / stride 2 / pad 1 depthwise: deconv_dw_up2_kernel past its first x-block of 256 columns (W = 257: one lane in the second
    block; W = 300: ragged), on one row, one column and one channel, against deconv_dw_kernel (y one float into a larger buffer)
    bit for bit, and against the oracle within 1e-6."""
    rng = np.random.default_rng(51)
    N, Cc, H, W = shape
    x = rng.standard_normal(shape).astype(np.float32)
    w = (orc.bilinear_filler((Cc, 1, 4, 4)) * rng.uniform(0.5, 1.5, (Cc, 1, 4, 4))).astype(np.float32)
    b = rng.standard_normal(Cc).astype(np.float32) if bias else None
    bd = None if b is None else dev(b)
    quad = hip.deconv_depthwise(dev(x), dev(w), bd, (1, 1), (2, 2)).cpu().numpy()
    per_output = deconv_dw_into(hip, dev(x), dev(w), bd, shifted_empty((N, Cc, 2 * H, 2 * W)), (1, 1), (2, 2)).cpu().numpy()
    assert quad.tobytes() == per_output.tobytes()
    close(quad, orc.deconv2d(x, w, b, (1, 1), (2, 2), group=Cc), 1e-6)


def test_deconv_depthwise_more_planes_than_a_grid_dimension(hip, orc):
    """N * C = 65 536 planes do not fit blockIdx.z: the 4x4 / stride 2 / pad 1 case falls back to the per-output kernel."""
    rng = np.random.default_rng(52)
    x = rng.standard_normal((2, 32768, 2, 2)).astype(np.float32)
    w = rng.standard_normal((32768, 1, 4, 4)).astype(np.float32)
    close(hip.deconv_depthwise(dev(x), dev(w), None, (1, 1), (2, 2)).cpu().numpy(), orc.deconv2d(x, w, None, (1, 1), (2, 2), group=32768), 1e-6)


def test_deconv_groups_kernels_strides_pads_bias(hip, orc):
    """The cases of the CPU pin (groups 1, 2 and Cin with Cout != Cin, depthwise; kernels (3,5) (5,3) (1,1); strides (1,3) (3,2);
    pad 0 and kernel // 2; with and without bias) through mscnn_deconv2d_fwd_f32."""
    for i, case in enumerate(sc.deconv_cases()):
        x, w, b, g = sc.deconv_inputs(case, i)
        y = hip.deconv2d(dev(x), dev(w), None if b is None else dev(b), case[3], case[2], g).cpu().numpy()
        close(y, orc.deconv2d(x, w, b, case[3], case[2], g), 1e-6 if case[0] == "dw" else 1e-4)


# ------------------------------------------------------------------------------------------------ ReLU
def test_relu_special_values_have_the_reference_bit_patterns(hip):
    """+-0, +-inf and NaN at slopes 0, 0.1 and -0.5 against the values recorded from the reference (tests/golden/make_golden_c.py):
    the float4 kernel, the scalar kernel (count % 4 != 0, and an unaligned base) and in place."""
    import os
    G = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_layers_c.npz"))
    x = sc.RELU_SPECIALS_DEVICE
    assert np.array_equal(sc.bits(G["relu_x"][:x.size]), sc.bits(x))
    for slope, want in zip(sc.RELU_SLOPES, G["relu_y"]):
        want = sc.bits(want[:x.size])
        x4 = np.tile(x, 4)                                                        # 20 floats, aligned: relu_kernel_v4
        assert np.array_equal(sc.bits(hip.relu(dev(x4), slope).cpu().numpy()), np.tile(want, 4)), slope
        assert np.array_equal(sc.bits(hip.relu(dev(x), slope).cpu().numpy()), want), slope          # 5 floats: relu_kernel
        assert np.array_equal(sc.bits(hip.relu(shifted(x4), slope).cpu().numpy()), np.tile(want, 4)), slope
        for t in (dev(x4), dev(x)):
            hip.relu(t, slope, inplace=True)
            assert np.array_equal(sc.bits(t.cpu().numpy()), np.tile(want, t.numel() // x.size)), slope


# ------------------------------------------------------------------------------------------------ Softmax, Eltwise
def test_softmax_shapes_scales_and_special_rows(hip, orc):
    for tag, x in sc.softmax_inputs():
        y = hip.softmax(dev(x)).cpu().numpy()
        ref = orc.softmax(x)
        assert np.array_equal(np.isnan(y), np.isnan(ref)), tag
        assert np.allclose(y, ref, rtol=0, atol=1e-6, equal_nan=True), tag
        sums = y.astype(np.float64).sum(1)
        finite = np.isfinite(x).all(1)
        assert finite.any() or x.shape == (1, 5, 1, 1), tag                      # (that shape has one row: the special one)
        assert not finite.any() or np.abs(sums[finite] - 1).max() <= 1e-6, tag
        assert np.isnan(sums[~finite]).all(), tag


def test_eltwise_bottom_counts_and_ties(hip, orc):
    for nb in sc.ELTWISE_BOTTOMS:
        xs = sc.eltwise_inputs(nb, (37, 5))
        ds = [dev(x) for x in xs]
        for op, cf in (("PROD", None), ("SUM", None), ("MAX", None), ("SUM", sc.ELTWISE_COEFFS[nb])):
            assert np.array_equal(hip.eltwise(ds, op, cf).cpu().numpy(), orc.eltwise(xs, op, cf)), (nb, op, cf)


# ------------------------------------------------------------------------------------------------ the Pooling host layer
POOL_LAYER_FORMS = {
    "h_w_forms": ((2, 3, 9, 11), "pool: AVE kernel_h: 3 kernel_w: 2 pad_h: 1 pad_w: 0 stride_h: 2 stride_w: 3"),
    "one_pad_clips_both": ((1, 2, 3, 4), "pool: MAX kernel_h: 1 kernel_w: 2 pad_h: 0 pad_w: 1 stride_h: 3 stride_w: 1"),
    "one_pad_clips_both_ave": ((1, 2, 3, 4), "pool: AVE kernel_h: 1 kernel_w: 2 pad_h: 0 pad_w: 1 stride_h: 3 stride_w: 1"),
    "global_max": ((2, 3, 5, 7), "pool: MAX global_pooling: true"),
    "global_ave": ((2, 3, 5, 7), "pool: AVE global_pooling: true"),
    "square": ((1, 2, 7, 8), "pool: MAX kernel_size: 3 pad: 1 stride: 2"),
}


def pool_net_text(shape, param):
    dims = " ".join(f"input_dim: {d}" for d in shape)
    return f'name: "p" input: "data" {dims} layer {{ name: "pool" type: "Pooling" bottom: "data" top: "pool" pooling_param {{ {param} }} }}'


@pytest.mark.parametrize("form", sorted(POOL_LAYER_FORMS))
def test_pooling_layer_parameter_forms(hip, orc, form):
    """A one-layer Net per parameter form: the top's shape and values are the oracle executor's (which reads the same text)."""
    from mscnn_amd import net as mnet
    from oracle import pynet
    shape, param = POOL_LAYER_FORMS[form]
    n = mnet.Net(prototxt_text=pool_net_text(shape, param))
    x = np.random.default_rng(61).standard_normal(shape).astype(np.float32)
    n.set_blob("data", x)
    n.forward()
    layers = [(n.layer_names[i], n.layer_types[i], n.layer_bottoms(i), n.layer_tops(i), n.layer_param_text(i)) for i in range(len(n.layer_names))]
    ref = pynet.forward(layers, {}, {"data": x})["pool"]
    if form.startswith("one_pad"):
        assert ref.shape == (1, 2, 1, 5)
    if form.startswith("global"):
        assert ref.shape == shape[:2] + (1, 1)
    y = n.get_blob("pool")
    assert tuple(n.blob_shape("pool")) == ref.shape == y.shape
    if "MAX" in param:
        assert np.array_equal(y, ref)
    else:
        check_ave(y, ref, form)

