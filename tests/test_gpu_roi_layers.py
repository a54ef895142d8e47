"""The ROI and box-decode ops on the GPU through every branch of their kernels, against the oracle that tests/test_oracle_vs_ref.py pins
to the reference: ROIPooling's row kernel (slot widths 8 .. 128, two columns per lane, column segments, the row tail, 256 bins, channel
groups of more than one round), its per-bin fallback, the pair op in one and in two launches, the fused pooling + F(3x3,3x3) input
transform against the unfused sequence, ROIAlign and its one-pass AVE forms, and DecodeBBox with its exponent range.  The cases are
tests/roi_cases.py's; tests/test_roi_cases_cpu.py shows from the geometry restatement that they reach every branch named here.

Comparison: on the plain and the post-ReLU map bit for bit.  On the special map (NaN, +-inf, -FLT_MAX-scale, signed zeros) NaN
positions are identical, every other value is equal under ==, and every non-zero expected value is bit-identical -- the sign of a zero
is not compared there (the row kernel's order of comparisons can return the other zero of a -0 / +0 tie).  NaN payloads are never
compared."""
import ctypes as C

import numpy as np
import pytest

import roi_cases as rc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BIT17 = 1 << 17           # ConvPlan tune_flags: uniform (not ragged) Winograd planes
POISON = 12345.0


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X: torch.cuda.is_available() is False")
    from mscnn_amd import hipapi
    hipapi.lib()
    return hipapi


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cpu(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def same(kind, got, want, what):
    got = np.asarray(got); want = np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if kind != "special":
        bad = rc.bits(got) != rc.bits(want)
        assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])
        return
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaN positions")
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok], want[ok]), (what, "values")
    nz = ok & (want != 0)
    assert np.array_equal(got[nz].view(np.uint32), want[nz].view(np.uint32)), (what, "bits of non-zero values")


_MAPS = {}


def fmap(kind, shape):
    key = (kind, shape)
    if key not in _MAPS:
        a = rc.feature_map(kind, shape)
        d = dev(a)
        a.setflags(write=False)
        _MAPS[key] = (a, d)
    return _MAPS[key]


# ------------------------------------------------------------------------------------------------ ROIPooling: the row kernel
@pytest.mark.parametrize("size", rc.ROW_SIZES)
def test_roipool_row_kernel_every_case(hip, orc, size):
    """mscnn_roipool_fwd_f32 at every case of roi_cases.row_cases() with this pooled size, on all three maps (C = 5 on the small map:
    chan_per_block capped by C or a partial last group; 8 on the wide and the tall one)."""
    n = 0
    for tag, mk, rois, PH, PW, scale, pad in rc.row_cases():
        if (PH, PW) != size:
            continue
        rd = dev(rois)
        for kind in rc.MAP_KINDS:
            feat, fd = fmap(kind, rc.case_shape(mk, 5))
            same(kind, cpu(hip.roipool(fd, rd, PH, PW, scale, pad)), orc.roipool(feat, rois, PH, PW, scale, pad), (tag, kind))
            n += 1
    assert n >= 27


@pytest.mark.parametrize("Cc", [c for c in rc.ROW_CHANNELS if c != 5])
def test_roipool_row_kernel_channel_groups(hip, orc, Cc):
    """C = 1, 24, 128 (the 16-channel groups) and 200 (more channels than one round of slots; a partial last group) at every pooled
    size; scale, pad and map rotate over the sizes."""
    combos = [(s, p) for s in rc.SCALES for p in rc.PADS]
    for i, (PH, PW) in enumerate(rc.ROW_SIZES):
        scale, pad = combos[(i + Cc) % len(combos)]
        kind = rc.MAP_KINDS[(i + Cc) % 3]
        rois = rc.std_rois(*rc.STD_HW, 2, scale, seed=Cc)
        feat, fd = fmap(kind, rc.std_shape(Cc))
        same(kind, cpu(hip.roipool(fd, dev(rois), PH, PW, scale, pad)), orc.roipool(feat, rois, PH, PW, scale, pad), (Cc, PH, PW, scale, pad, kind))


def test_roipool_row_kernel_channel_window(hip, orc):
    """c_total / c_offset: the row kernel writes its window of the output and nothing else (wide map: the segment accumulation reads
    its own earlier stores back)."""
    for mk, rois, PH, PW, scale, pad in [("std", rc.std_rois(*rc.STD_HW, 2, 0.25), 6, 7, 0.25, 0.5), ("wide", rc.wide_rois(1.0), 3, 5, 1.0, 0.0)]:
        feat, fd = fmap("plain", rc.case_shape(mk, 5))
        Cc = feat.shape[1]
        out = torch.full((len(rois), Cc + 7, PH, PW), POISON, dtype=torch.float32, device="cuda")
        hip.roipool(fd, dev(rois), PH, PW, scale, pad, out=out, c_total=Cc + 7, c_offset=3)
        o = cpu(out)
        same("plain", o[:, 3:3 + Cc], orc.roipool(feat, rois, PH, PW, scale, pad), mk)
        assert (o[:, :3] == POISON).all() and (o[:, 3 + Cc:] == POISON).all()


# ------------------------------------------------------------------------------------------------ ROIPooling: the per-bin kernel
@pytest.mark.parametrize("Cc", rc.PERBIN_CHANNELS)
@pytest.mark.parametrize("size", rc.PERBIN_SIZES)
def test_roipool_per_bin_kernel(hip, orc, size, Cc):
    """pooled_h or pooled_w above 16: roipool_kernel, every scale and pad on all three maps, and through a c_total / c_offset window
    between poisoned neighbours."""
    PH, PW = size
    for si, scale in enumerate(rc.SCALES):
        rois = rc.std_rois(*rc.STD_HW, 2, scale, seed=si)
        rd = dev(rois)
        for pi, pad in enumerate(rc.PADS):
            kind = rc.MAP_KINDS[(si + pi) % 3] if Cc == 128 else None
            for k in ([kind] if kind else rc.MAP_KINDS):
                feat, fd = fmap(k, rc.std_shape(Cc))
                same(k, cpu(hip.roipool(fd, rd, PH, PW, scale, pad)), orc.roipool(feat, rois, PH, PW, scale, pad), (PH, PW, scale, pad, k))
    feat, fd = fmap("special", rc.std_shape(Cc))
    out = torch.full((len(rois), Cc + 5, PH, PW), POISON, dtype=torch.float32, device="cuda")
    hip.roipool(fd, rd, PH, PW, scale, 0.5, out=out, c_total=Cc + 5, c_offset=2)
    o = cpu(out)
    same("special", o[:, 2:2 + Cc], orc.roipool(feat, rois, PH, PW, scale, 0.5), "window")
    assert (o[:, :2] == POISON).all() and (o[:, 2 + Cc:] == POISON).all()


# ------------------------------------------------------------------------------------------------ ROIPooling: the pair op
def _pair(hip, fd, rd, PH, PW, scale, pad_a, off_a, pad_b, off_b, c_total):
    N, Cc, H, W = fd.shape
    out = torch.full((rd.shape[0], c_total, PH, PW), POISON, dtype=torch.float32, device="cuda")
    hip._check(hip.lib().mscnn_roipool_pair_fwd_f32(hip._dev(fd), hip._dev(rd), hip._dev(out), rd.shape[0], N, Cc, H, W, PH, PW, C.c_float(scale),
                                                    C.c_float(pad_a), off_a, C.c_float(pad_b), off_b, c_total, hip._stream()))
    return cpu(out)


@pytest.mark.parametrize("size", rc.PAIR_SIZES)
def test_roipool_pair(hip, orc, size):
    """mscnn_roipool_pair_fwd_f32 (roipool_rows_kernel<2>; (17, 7): its two-launch fallback through roipool_kernel): both pad orders,
    pad_a == pad_b, adjacent and non-adjacent channel windows with poison between them; the wide map's context window needs more
    segments and a wider slot than the ROI's own."""
    PH, PW = size
    for i, (mk, rois, scale, Cc) in enumerate(rc.pair_sets(PH)):
        rd = dev(rois)
        for j, (pad_a, pad_b) in enumerate(rc.pair_pads(mk)):
            kind = rc.MAP_KINDS[(i + j) % 3]
            feat, fd = fmap(kind, rc.case_shape(mk, Cc))
            Cm = feat.shape[1]
            wa, wb = orc.roipool(feat, rois, PH, PW, scale, pad_a), orc.roipool(feat, rois, PH, PW, scale, pad_b)
            what = (mk, PH, PW, scale, pad_a, pad_b, kind)
            if j % 2 == 0:      # adjacent windows, a first: the Python wrapper
                same(kind, cpu(hip.roipool_pair(fd, rd, PH, PW, scale, pad_a, pad_b)), np.concatenate([wa, wb], 1), what)
            else:               # b first, a gap of 3 channels between the windows and 2 behind
                off_b, off_a, tot = 0, Cm + 3, 2 * Cm + 5
                o = _pair(hip, fd, rd, PH, PW, scale, pad_a, off_a, pad_b, off_b, tot)
                same(kind, o[:, off_a:off_a + Cm], wa, what + ("a",))
                same(kind, o[:, off_b:off_b + Cm], wb, what + ("b",))
                assert (o[:, Cm:Cm + 3] == POISON).all() and (o[:, 2 * Cm + 3:] == POISON).all(), what


# ------------------------------------------------------------------------------------------------ fused pooling + transform
def _fused_plan(hip, R, Cc, Cout, flags=0):
    rng = np.random.default_rng(100 + R)
    w = (rng.standard_normal((Cout, 2 * Cc, 3, 3)) * np.sqrt(2.0 / (2 * Cc * 9))).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32)
    plan = hip.ConvPlan(R, 2 * Cc, 7, 7, Cout, 3, 3, (0, 0), relu=True, algo=hip.ALGO_WINO_F3, tune_flags=flags)
    assert plan.kernel == "winograd_f3x3_3x3" and plan.can_fuse_roipool(Cc, 7, 7), plan.kernel
    plan.pack(dev(w))
    return plan, dev(b)


def _ragged(plan):
    cols = plan.plane_columns()
    return cols != [cols[0]] * len(cols)


@pytest.mark.parametrize("R,batch,H8,W8", [(8, 1, 24, 40), (13, 2, 24, 40), (45, 2, 20, 28)])
def test_fused_roipool_transform_every_branch(hip, orc, R, batch, H8, W8):
    """forward_roipool_pair (roipool_wino33_kernel) at the smallest plan that fuses (C = 64, R >= 8; R = 13 and 45 leave a partial last
    workgroup) on a ROI set whose census shows every level k = 0 .. 3 with `wide` true and false, the extra-squares loop and empty
    bins on each side: y equals the unfused sequence's as bit patterns, with ragged and with uniform planes, and the unfused pooled
    blob equals the oracle's for ALL ROIs."""
    Cc, Cout = 64, 64
    rois = rc.fused_rois(H8, W8, batch, R)
    rd = dev(rois)
    plans = [_fused_plan(hip, R, Cc, Cout), _fused_plan(hip, R, Cc, Cout, BIT17)]
    print(f"R={R}: planes ragged = {[_ragged(p) for p, _ in plans]}")
    assert not _ragged(plans[1][0])
    for kind in ("relu", "plain"):
        feat, fd = fmap(kind, (batch, Cc, H8, W8))
        pooled = hip.roipool_pair(fd, rd, 7, 7, 0.125, 0.0, 0.25)
        want = np.concatenate([orc.roipool(feat, rois, 7, 7, 0.125, 0.0), orc.roipool(feat, rois, 7, 7, 0.125, 0.25)], 1)
        same(kind, cpu(pooled), want, (kind, "pooled"))
        for plan, bd in plans:
            y_ref = plan.forward(pooled, bd).clone()
            y = plan.forward_roipool_pair(fd, rd, 0.125, 0.0, 0.25, bd)
            assert np.array_equal(rc.bits(cpu(y)), rc.bits(cpu(y_ref))), (kind, _ragged(plan))


def _nan_lattice_map(shape):
    """Post-ReLU, with a NaN in one cell of five, placed so that every 2 x 2 square holds finite cells: NaN cells are the ANCHORS
    (top-left cells) of squares whose maximum lies elsewhere in the square."""
    N, Cc, H, W = shape
    x = rc.feature_map("relu", shape, seed=5) + np.float32(0.25)
    n, c, h, w = np.meshgrid(np.arange(N), np.arange(Cc), np.arange(H), np.arange(W), indexing="ij")
    x[(h + 2 * w + c + n) % 5 == 0] = np.nan
    return x


def _sliding_max_ref(feat):
    """[4][N][H][W][C]: the channel-last map and its sliding maxima over 2 x 2, 4 x 4, 8 x 8 squares (clamped at the border), a NaN
    cell skipped as the reference's scan skips it (-FLT_MAX where a square holds nothing else)."""
    lv = [np.ascontiguousarray(feat.transpose(0, 2, 3, 1))]
    N, H, W, Cc = lv[0].shape
    for k in range(1, 4):
        half = 1 << (k - 1)
        s = lv[-1]
        y2 = np.minimum(np.arange(H) + half, H - 1); x2 = np.minimum(np.arange(W) + half, W - 1)
        m = np.full_like(s, -rc.FLT_MAX)
        for t in (s, s[:, :, x2], s[:, y2], s[:, y2][:, :, x2]):
            m = np.where(t > m, t, m)                                    # (a NaN compares false: skipped)
        lv.append(m)
    return np.stack(lv)


def test_fused_level_maps(hip):
    """mscnn_roipool_maps_build_f32 against a numpy sliding maximum: bit for bit on a finite post-ReLU map (what every level held
    before NaN cells were skipped, too: a plain maximum), and on the NaN-lattice map every level above 0 is the maximum of the
    square's finite cells."""
    shape = (2, 64, 20, 28)
    for name, feat in [("relu", rc.feature_map("relu", shape)), ("nan", _nan_lattice_map(shape))]:
        got = cpu(hip.roipool_maps(dev(feat))).reshape((4, shape[0], shape[2], shape[3], shape[1]))
        want = _sliding_max_ref(feat)
        if name == "relu":
            assert np.isfinite(want).all()
        else:
            # (the clamped square of the map's last cell is that cell alone: -FLT_MAX where it is NaN)
            assert np.isnan(want[0]).mean() > 0.15 and not np.isnan(want[1:]).any() and (want[1:] > 0).mean() > 0.99
        assert np.array_equal(rc.bits(got), rc.bits(want)), name


def test_fused_roipool_skips_nan_cells_like_the_unfused_path(hip, orc):
    """A post-ReLU map with NaN cells at the anchors of squares whose true maximum lies elsewhere: the reference's scan (and the row
    kernel) skip the NaN cell and keep the square's finite values, so must the level maps the fused kernel reads.  Fused and unfused
    y as bit patterns; the unfused pooled blob against the oracle."""
    R, batch, H8, W8, Cc, Cout = 13, 2, 24, 40, 64, 64
    feat = _nan_lattice_map((batch, Cc, H8, W8))
    rois = rc.fused_rois(H8, W8, batch, R)
    fd, rd = dev(feat), dev(rois)
    plan, bd = _fused_plan(hip, R, Cc, Cout)
    pooled = hip.roipool_pair(fd, rd, 7, 7, 0.125, 0.0, 0.25)
    want = np.concatenate([orc.roipool(feat, rois, 7, 7, 0.125, 0.0), orc.roipool(feat, rois, 7, 7, 0.125, 0.25)], 1)
    assert not np.isnan(want).any() and (want > 0).mean() > 0.4          # NaN never wins a bin; most bins hold finite maxima
    same("relu", cpu(pooled), want, "pooled")
    y_ref = plan.forward(pooled, bd).clone()
    y = plan.forward_roipool_pair(fd, rd, 0.125, 0.0, 0.25, bd)
    bad = rc.bits(cpu(y)) != rc.bits(cpu(y_ref))
    assert not bad.any(), (int(bad.sum()), bad.size)
    # (a one-cell bin on a NaN cell is -FLT_MAX on both paths and overflows in the transform: most ROIs have none, their y is finite)
    clean = ~(want == -rc.FLT_MAX).any((1, 2, 3))
    assert clean.sum() >= 8 and np.isfinite(cpu(y_ref)[clean]).all()


# ------------------------------------------------------------------------------------------------ ROIAlign
@pytest.mark.parametrize("size", rc.ALIGN_SIZES)
def test_roialign(hip, orc, size):
    """mscnn_roialign_fwd_f32: C = 5 at every scale and pad on all three maps (the operation order is the oracle's, so NaN and inf
    propagate to the same positions), C = 1, 24 and 128 with scale, pad and map rotating."""
    PH, PW = size
    combos = [(s, p) for s in rc.SCALES for p in rc.PADS]
    for ci, (scale, pad) in enumerate(combos):
        rois = rc.std_rois(*rc.STD_HW, 2, scale, seed=ci % 3)
        rd = dev(rois)
        for Cc in rc.ALIGN_CHANNELS:
            for kind in (rc.MAP_KINDS if Cc == 5 else [rc.MAP_KINDS[(ci + Cc) % 3]]):
                if Cc != 5 and (ci + Cc + PH) % 3:
                    continue
                feat, fd = fmap(kind, rc.std_shape(Cc))
                same(kind, cpu(hip.roialign(fd, rd, PH, PW, scale, pad)), orc.roialign(feat, rois, PH, PW, scale, pad), (PH, PW, Cc, scale, pad, kind))


def test_roialign_ave_largest_grid_and_refusal(hip, orc):
    """mscnn_roialign_ave_fwd_f32 and its pair at 15 x 15 bins (256 grid points: one slot of the workgroup), C = 24; 16 x 15 is a grid
    of 272 points and is refused, naming the sizes, with the output untouched."""
    scale = 0.25
    rois = rc.std_rois(*rc.STD_HW, 2, scale)
    rd = dev(rois)
    for kind in ("plain", "relu"):
        feat, fd = fmap(kind, rc.std_shape(24))
        win = {p: orc.pool2d(orc.roialign(feat, rois, 15, 15, scale, p), (2, 2), (0, 0), (1, 1), "AVE") for p in (0.0, 0.5)}
        same(kind, cpu(hip.roialign_ave(fd, rd, 15, 15, scale, 0.5)), win[0.5], (kind, "single"))
        same(kind, cpu(hip.roialign_ave_pair(fd, rd, 15, 15, scale, 0.0, 0.5)), np.concatenate([win[0.0], win[0.5]], 1), (kind, "pair"))
    out = torch.full((len(rois), 48, 16, 15), POISON, dtype=torch.float32, device="cuda")
    for call in (lambda: hip.roialign_ave(fd, rd, 16, 15, scale, 0.5, out=out, c_total=48),
                 lambda: hip.roialign_ave_pair(fd, rd, 16, 15, scale, 0.0, 0.5, out=out)):
        with pytest.raises(hip.MscnnError, match=r"16 x 15"):
            call()
    assert (cpu(out) == POISON).all()


# ------------------------------------------------------------------------------------------------ DecodeBBox
def _exponents(bbox, mean, std):
    return bbox[:, 6:8] * np.array(std[2:], np.float32) + np.array(mean[2:], np.float32)


def _classes(a):
    """finite non-zero / zero / +inf / -inf / NaN, as small integers"""
    return np.select([np.isnan(a), np.isposinf(a), np.isneginf(a), a == 0], [4, 3, 2, 1], 0)


def _ulps(a, b):
    def key(v):
        i = v.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


@pytest.mark.parametrize("R", rc.DECODE_ROWS)
def test_decode_bbox_parameter_sets(hip, orc, R):
    """mscnn_decodebbox_fwd_f32 at R = 1, 255, 256, 257 (the last lane of a workgroup, the first of the next) and every parameter set.
    Rows whose exponents are all inside (-87, 87): bit for bit.  The others (|x| >= 87, inf, NaN: device libm, the class of the result
    is what is promised): finite / zero / inf / NaN where the oracle has it."""
    bbox, prior = rc.decode_inputs(R)
    for name, (mean, std) in rc.DECODE_PARAMS.items():
        want = orc.decode_bbox(bbox, prior, mean, std)
        got = cpu(hip.decode_bbox(dev(bbox), dev(prior), mean, std))
        e = _exponents(bbox, mean, std)
        inside = (np.abs(e) < 87).all(1) & np.isfinite(bbox[:, 4:]).all(1)
        assert np.array_equal(rc.bits(got[inside]), rc.bits(want[inside])), name
        assert np.array_equal(_classes(got[~inside]), _classes(want[~inside])), name
        if R >= 64:
            assert (~inside).sum() >= 4 and np.isnan(want).any() and np.isinf(want).any(), name


def test_decode_bbox_exponent_sweep(hip, orc):
    """2^18 rows, std 1, mean 0: both exponents cover (-87, 87) densely (no gap wider than 0.002), prior sizes 1, 37.5 and 1024 --
    expf_libm's promise of glibc's bits, held on the device.  Bit for bit."""
    bbox, prior = rc.decode_sweep()
    want = orc.decode_bbox(bbox, prior)
    got = cpu(hip.decode_bbox(dev(bbox), dev(prior)))
    bad = (rc.bits(got) != rc.bits(want)).any(1)
    assert not bad.any(), (int(bad.sum()), bbox[bad][:4, 6:], got[bad][:4], want[bad][:4])


def test_decode_bbox_beyond_the_table_range(hip, orc):
    """87 <= |x| <= 110: the header promises nothing about the bits.  The class of every output is the oracle's; the largest distance
    in ulps is printed (profiles/roi_layers_tests.txt keeps the figure measured when this test was written)."""
    bbox, prior = rc.decode_beyond()
    want = orc.decode_bbox(bbox, prior)
    got = cpu(hip.decode_bbox(dev(bbox), dev(prior)))
    assert np.array_equal(_classes(got), _classes(want))
    fin = np.isfinite(want) & (want != 0)
    d = _ulps(got[fin], want[fin])
    print(f"decode_bbox, 87 <= |x| <= 110: {int(fin.sum())} finite non-zero outputs, largest distance {int(d.max())} ulp, "
          f"{int((d > 0).sum())} differ; classes (finite, zero, +inf, -inf, NaN) = {np.bincount(_classes(want).reshape(-1), minlength=5).tolist()}")


@pytest.mark.parametrize("std", rc.DECODE_REFUSED_STD)
def test_decode_bbox_refuses_std_not_above_zero(hip, std):
    """decode_bbox_layer.cpp:30: a std that is zero, negative, -0 or NaN is refused before any launch; the message names the element
    and its value."""
    bbox, prior = rc.decode_inputs(16)
    out_before = None
    with pytest.raises(hip.MscnnError, match=r"bbox_std\[\d\] = \S+ must be > 0") as ei:
        out_before = hip.decode_bbox(dev(bbox), dev(prior), (0, 0, 0, 0), std)
    assert out_before is None
    k = next(i for i in range(4) if not std[i] > 0)
    assert f"bbox_std[{k}]" in str(ei.value)
