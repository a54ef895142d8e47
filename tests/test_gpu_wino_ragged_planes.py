"""Ragged planes of the small-map F(3x3,3x3) layers on the GPU (tests/test_wino_ragged_planes_model.py has the rule and the
schedule on the host): the layer with per-plane tile grids against the same layer with uniform planes (tune_flags bit 17).  Every
kept output is the same fp32 expression over the same operands, so with whole GEMM tiles the results are BIT-IDENTICAL; with the
stream-K split a tile's chunks are summed in parts, within the split tolerance of test_wgemm_plane_gemm_against_the_igemm_kernel."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BIT17 = 1 << 17
WHOLE, SPLIT = 512, 256


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X: torch.cuda.is_available() is False")
    from mscnn_amd import hipapi
    hipapi.lib()
    return hipapi


def _data(case):
    R, Cin, H, W, Cout, pad = case
    g = torch.Generator(device="cuda").manual_seed(1000 + R)
    x = torch.relu(torch.randn((R, Cin, H, W), device="cuda", generator=g))
    w = torch.randn((Cout, Cin, 3, 3), device="cuda", generator=g) * (2.0 / (Cin * 9)) ** 0.5
    b = torch.randn((Cout,), device="cuda", generator=g)
    return x, w, b


def _plan(hip, case, w, tune_variant, tune_flags=0):
    R, Cin, H, W, Cout, pad = case
    p = hip.ConvPlan(R, Cin, H, W, Cout, 3, 3, (pad, pad), relu=True, algo=hip.ALGO_WINO_F3, tune_variant=tune_variant, tune_flags=tune_flags)
    assert p.kernel == "winograd_f3x3_3x3"
    p.pack(w)
    return p


def _is_ragged(p):
    cols = p.plane_columns()
    return cols != [cols[0]] * len(cols)


def _rel(a, r):
    return ((a.double() - r.double()).abs() / torch.clamp(r.double().abs(), min=1.0)).max().item()


# R, Cin, H, W, Cout, pad, ragged: rows past Cout and one column tile per plane | 9 / 5 / 3 column tiles | only i == 4 shortened
# (Cout = 40 is no multiple of 32: that plan keeps the igemm GEMM and uniform planes; Cout = 64 runs the ragged form) | both axes and
# a tile with one valid column | whole tiles: the plan reports uniform planes | a small map with pad 2: a 10 x 10 / 10 x 9 output, beyond
# the LDS-staged output kernel's maps -- the generic output kernel reads the ragged planes
CASES = [((9, 32, 8, 8, 64, 2), True), ((12, 32, 8, 7, 64, 2), True), ((9, 64, 7, 7, 96, 0), True), ((257, 64, 7, 7, 96, 0), True), ((37, 32, 7, 5, 40, 0), False), ((37, 32, 7, 5, 64, 0), True),
         ((130, 32, 8, 4, 64, 1), True), ((20, 64, 6, 6, 48, 1), False)]


@pytest.mark.parametrize("case,ragged", CASES)
def test_ragged_against_uniform_planes_same_bits(hip, case, ragged):
    x, w, b = _data(case)
    pr, pu = _plan(hip, case, w, 300 + WHOLE), _plan(hip, case, w, 300 + WHOLE, BIT17)
    assert _is_ragged(pr) == ragged and not _is_ragged(pu)
    yr, yu = pr.forward(x, b).clone(), pu.forward(x, b).clone()
    assert torch.equal(yr, yu)
    # the generic per-tile output transform (bit 8) reads the same ragged planes
    assert torch.equal(_plan(hip, case, w, 300 + WHOLE, 256).forward(x, b), yu)
    pad = case[5]
    ref = torch.relu(torch.nn.functional.conv2d(x.double(), w.double(), b.double(), padding=pad))
    assert _rel(yr, ref) < 1e-4


@pytest.mark.parametrize("variant", [3, 4, 5])
def test_ragged_against_uniform_planes_other_tile_shapes(hip, variant):
    """128 x 128, 256 x 96 and 256 x 160 tiles (B pieces that straddle rows) on the 9 / 5 / 3 column-tile case."""
    case = (257, 64, 7, 7, 96, 0)
    x, w, b = _data(case)
    pr, pu = _plan(hip, case, w, 300 + variant + WHOLE), _plan(hip, case, w, 300 + variant + WHOLE, BIT17)
    assert _is_ragged(pr) and not _is_ragged(pu)
    assert torch.equal(pr.forward(x, b), pu.forward(x, b))


@pytest.fixture(scope="module")
def split_case(hip):
    case = (130, 1024, 7, 7, 512, 0)
    x, w, b = _data(case)
    y_whole = _plan(hip, case, w, 300 + WHOLE).forward(x, b).clone()
    ref = torch.relu(torch.nn.functional.conv2d(x.double(), w.double(), b.double()))
    return case, x, w, b, y_whole, ref


@pytest.mark.parametrize("tune_variant", [300 + SPLIT, 0])
def test_ragged_split_schedule(hip, split_case, tune_variant):
    """The stream-K split (forced, and the plan's own schedule) on ragged planes: within 4e-5 of the whole-tile result (relative to
    max(1, |y|)), the same bits from run to run, within 1e-4 of the float64 convolution; no hand-off timed out."""
    case, x, w, b, y_whole, ref = split_case
    before = hip.wgemm_handoff_event()
    p = _plan(hip, case, w, tune_variant)
    assert _is_ragged(p)
    y = p.forward(x, b).clone()
    err = _rel(y, y_whole)
    print(f"split vs whole {err:.2e}  vs float64 {_rel(y, ref):.2e}")
    assert err < 4e-5, err
    for _ in range(3):
        assert torch.equal(p.forward(x, b), y)
    assert _rel(y, ref) < 1e-4
    torch.cuda.synchronize()
    assert hip.wgemm_handoff_event() == before


def test_ragged_planes_ignore_a_stale_workspace(hip):
    """Forward at R = 257, then set_batch(37) on the same plan (the workspace keeps the larger frame's planes): the result equals a
    fresh plan's at R = 37 -- no output transform reads a column beyond a plane's live ones."""
    case = (257, 64, 7, 7, 96, 0)
    x, w, b = _data(case)
    p = _plan(hip, case, w, 300 + WHOLE)
    p.forward(x, b)
    p.set_batch(37)
    assert _is_ragged(p)
    x37 = x[:37].contiguous()
    y = p.forward(x37, b).clone()
    fresh = _plan(hip, (37,) + case[1:], w, 300 + WHOLE)
    assert torch.equal(y, fresh.forward(x37, b))


def _kitti_like_rois(rng, R, H8, W8, batch=1):
    """Proposals as BoxOutput leaves them (image coordinates, stride-8 map): log-uniform widths, some leaving the image, some
    degenerate (zero / negative size), one covering everything."""
    w = np.exp(rng.uniform(np.log(6), np.log(8 * W8 * 0.9), R)); h = w * rng.uniform(0.3, 1.6, R)
    x1 = rng.uniform(-40, 8 * W8 - 10, R); y1 = rng.uniform(-30, 8 * H8 - 10, R)
    rois = np.stack([rng.integers(0, batch, R).astype(np.float64), x1, y1, x1 + w, y1 + h], 1).astype(np.float32)
    rois[3, 3] = rois[3, 1] - 5.0                  # x2 < x1
    rois[5, 1:] = [8 * W8 + 50, 10, 8 * W8 + 90, 60]      # entirely right of the map: every bin empty
    rois[7, 1:] = [-300, -200, 8 * W8 + 300, 8 * H8 + 200]   # covers everything
    return rois


@pytest.mark.parametrize("case", [(37, 64, 24, 40, 96), (133, 128, 36, 120, 64)])
def test_fused_roipool_writes_the_ragged_planes(hip, case):
    """The fused ROI pooling + input transform on a ragged plan against the unfused sequence through the same plan, and against
    the uniform plan (bit 17) with whole tiles: the same bits."""
    R, Cc, H8, W8, Cout = case
    rng = np.random.default_rng(R)
    feat = torch.from_numpy(np.maximum(rng.standard_normal((1, Cc, H8, W8)), 0).astype(np.float32) * 3.0).cuda()
    rois = torch.from_numpy(_kitti_like_rois(rng, R, H8, W8)).cuda()
    conv = (R, 2 * Cc, 7, 7, Cout, 0)
    _, w, b = _data(conv)
    p = _plan(hip, conv, w, 300 + WHOLE)
    assert _is_ragged(p) and p.can_fuse_roipool(Cc, 7, 7)
    pooled = hip.roipool_pair(feat, rois, 7, 7, 0.125, 0.0, 0.25)
    y_ref = p.forward(pooled, b).clone()
    assert torch.equal(p.forward_roipool_pair(feat, rois, 0.125, 0.0, 0.25, b), y_ref)
    pu = _plan(hip, conv, w, 300 + WHOLE, BIT17)
    assert torch.equal(pu.forward_roipool_pair(feat, rois, 0.125, 0.0, 0.25, b), y_ref)
