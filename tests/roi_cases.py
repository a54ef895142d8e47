"""The parameter space of the ROI layers (ROIPooling and its pair / fused forms, ROIAlign, DecodeBBox), stated once, in the pattern of
tests/stock_cases.py: tests/test_oracle_vs_ref.py sweeps it oracle against reference, tests/golden/make_golden_d.py records a subset
of it from the reference, tests/test_golden.py replays that subset, tests/test_roi_cases_cpu.py counts the kernel branches the case
lists reach and tests/test_gpu_roi_layers.py runs them HIP against oracle.

Inputs only.  Every function is deterministic in its arguments.  The one thing here that looks like an expectation is the GEOMETRY
restatement (window, bin_edges and the censuses built on them): numpy float32 forms of the reference's window and bin-edge
expressions (roi_pooling_layer.cu:33-59) that tell which BRANCH of which kernel a ROI takes.  It selects and counts cases; no output
value is ever compared with it, and tests/test_roi_cases_cpu.py holds it to the oracle.

Every ROI of every set has its batch index in [0, N) and finite coordinates below 1e6 in magnitude: outside that the reference's
int conversions are undefined and a batch index is an out-of-bounds read."""
import numpy as np

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max

# ------------------------------------------------------------------------------------------------ feature maps
STD_HW = (20, 33)             # the small map of most cases: 2 x C x 20 x 33
WIDE_SHAPE = (1, 8, 12, 300)  # spans of 65..128 (two columns per lane), 129..256 and > 256 columns (2 and 3 column segments)
TALL_SHAPE = (1, 8, 64, 16)   # bins of 6, 7, .. 11 and more rows: the row kernel's clamped 4-row tail with every remainder
MAP_KINDS = ("plain", "relu", "special")


def std_shape(C):
    return (2, C) + STD_HW


def feature_map(kind, shape, seed=0):
    """plain: signed normal values.  relu: post-ReLU, quantised to halves (plateaus of exactly equal values) with large zero regions.
    special: plain plus NaN cells, a whole-NaN plane, +-inf, -FLT_MAX-scale values and rows alternating -0 / +0."""
    N, C, H, W = shape
    rng = np.random.default_rng(9000 + 131 * seed + 7 * C + H + W)
    x = (rng.standard_normal(shape) * 2).astype(np.float32)
    if kind == "plain":
        return x
    if kind == "relu":
        x = (np.round(np.maximum(x, 0) * 2) / 2).astype(np.float32)
        x[:, :, H // 4:H // 2, W // 4:(3 * W) // 4] = 0
        x[:, ::2, :, :W // 8] = 0
        return x
    assert kind == "special", kind
    flat = x.reshape(-1)
    flat[3::37] = np.nan
    flat[5::53] = np.inf
    flat[11::59] = -np.inf
    flat[17::61] = -3e38
    x[:, :, 4, 0::2] = -0.0; x[:, :, 4, 1::2] = 0.0
    x[:, :, H - 3, 0::2] = 0.0; x[:, :, H - 3, 1::2] = -0.0
    x[N - 1, C - 1] = np.nan                       # a whole plane: every bin of it is -FLT_MAX or 0
    if C > 2:
        x[0, 1, :, :] = -np.inf
    return x


def positive_map(shape):
    """Strictly positive: a pooled bin is 0 exactly when it is empty."""
    return (np.abs(feature_map("plain", shape, seed=3)) + 1).astype(np.float32)


def bits(a):
    """Bit patterns with every NaN mapped to one pattern (NaN payloads differ between x86 and the device: never compared)."""
    a = np.ascontiguousarray(a, np.float32)
    u = a.view(np.uint32).copy()
    u[np.isnan(a)] = 0x7FC00000
    return u


# ------------------------------------------------------------------------------------------------ ROI sets
def _rows(rows, N):
    out = np.array(rows, np.float64).reshape(-1, 4)
    b = np.arange(len(out)) % N
    return np.concatenate([b[:, None].astype(np.float64), out], 1)


def hand_rois(H, W, N, scale):
    """The hand rows, in FEATURE cells here and divided by the scale below: [x1 y1 x2 y2]."""
    f = [
        (-300, 3, -200, 9), (W + 200, 3, W + 300, 9), (3, -300, 9, -200), (3, H + 200, 9, H + 300),      # far outside, each side
        (4, H + 5, 15, H + 9), (4, -12, 15, -6),                 # outside vertically only: a column span > 0, every bin empty
        (0, 0, W - 1, H - 1),                                    # the whole map
        (5, 7, 5, 7),                                            # a single point
        (12, 4, 6, 10), (6, 10, 12, 4), (12, 10, 6, 4),          # x2 < x1, y2 < y1, both
        (2.5, 1.5, 10.5, 6.5), (-1.5, -0.5, 7.5, 4.5), (-2.5, -3.5, W - 0.5, H - 1.5),      # edges exactly on .5 before roundf, +-
        (8, 8, 9, 9), (W - 2, H - 2, W - 1, H - 1),              # smaller than the pooled grid
        (-4, 5, 3, 12), (W - 4, 5, W + 5, 12), (6, -5, 14, 2), (6, H - 3, 14, H + 6),        # straddling each border
        (-6, -6, 2, 2), (W - 3, H - 3, W + 6, H + 6), (-20, -20, W + 20, H + 20),            # corners; wider than the map all round
    ]
    r = _rows(f, N)
    r[:, 1:] /= scale
    return r


def std_rois(H, W, N, scale, n_random=40, seed=0):
    """The hand rows plus random ROIs (log-uniform sizes from one cell to the whole map, most of them inside)."""
    rng = np.random.default_rng(7100 + seed)
    w = np.exp(rng.uniform(0, np.log(W), n_random)); h = np.exp(rng.uniform(0, np.log(H), n_random))
    x1 = rng.uniform(-0.1 * W, W - 0.6 * w); y1 = rng.uniform(-0.1 * H, H - 0.6 * h)
    rnd = np.stack([rng.integers(0, N, n_random).astype(np.float64), x1, y1, x1 + w, y1 + h], 1)
    rnd[:, 1:] /= scale
    out = np.concatenate([hand_rois(H, W, N, scale), rnd]).astype(np.float32)
    assert np.isfinite(out).all() and np.abs(out[:, 1:]).max() < 1e6 and out[:, 0].min() >= 0 and out[:, 0].max() < N
    return out


def wide_rois(scale=1.0):
    """For WIDE_SHAPE: spans of 65..128, 129..256 and more than 256 columns, at several heights and offsets, some leaving the map."""
    N, C, H, W = WIDE_SHAPE
    f = []
    for wd, x0 in [(64, 3), (65, 10), (100, 150), (128, 0), (129, 20), (200, 50), (256, 30), (257, 11), (290, 5), (299, 0), (340, -20),
                   (70, 260), (150, -40), (31, 7), (9, 200)]:
        for y0, ht in [(0, H - 1), (3, 4), (-5, 9)]:
            f.append((x0, y0, x0 + wd - 1, y0 + ht))
    r = _rows(f, N)
    r[:, 1:] /= scale
    return r.astype(np.float32)


def tall_rois(scale=1.0):
    """For TALL_SHAPE: every height from 1 to 70 rows (bins of 6, 7, .. 11 and more rows for pooled heights 1 .. 7), widths 1 .. 16."""
    N, C, H, W = TALL_SHAPE
    f = []
    for ht in range(1, 71):
        y0 = (ht * 5) % max(1, H - min(ht, H) + 1) - (3 if ht > 60 else 0)
        x0 = ht % 5 - 1
        f.append((x0, y0, x0 + 1 + ht % 14, y0 + ht - 1))
    r = _rows(f, N)
    r[:, 1:] /= scale
    return r.astype(np.float32)


# ------------------------------------------------------------------------------------------------ geometry restatement
def roundf(x):
    """C's roundf on float32: halves away from zero (np.round goes to even)."""
    x = np.asarray(x, np.float32)
    a = np.abs(x)
    fl = np.floor(a)
    r = fl + ((a - fl) >= f32(0.5)).astype(np.float32)          # a - floor(a) is exact
    return np.copysign(r, x).astype(np.int64)


def window(rois, scale, pad):
    """roi_pooling_layer.cu:33-41 in float32: (start_w, start_h, end_w, end_h, width, height), integer arrays of R."""
    rois = np.asarray(rois, np.float32)
    x1, y1, x2, y2 = (rois[:, k] for k in (1, 2, 3, 4))
    s, p = f32(scale), f32(pad)
    pad_w = (x2 - x1 + f32(1)) * p
    pad_h = (y2 - y1 + f32(1)) * p
    sw, sh = roundf((x1 - pad_w) * s), roundf((y1 - pad_h) * s)
    ew, eh = roundf((x2 + pad_w) * s), roundf((y2 + pad_h) * s)
    return sw, sh, ew, eh, np.maximum(ew - sw + 1, 1), np.maximum(eh - sh + 1, 1)


def bin_edges(start, size, P, limit):
    """roi_pooling_layer.cu:43-59 along one axis: clipped [lo, hi) of the P bins, integer arrays of R x P."""
    bin_size = (size.astype(np.float32) / f32(P))[:, None]
    p = np.arange(P, dtype=np.float32)[None, :]
    lo = np.floor(p * bin_size).astype(np.int64) + start[:, None]
    hi = np.ceil((p + f32(1)) * bin_size).astype(np.int64) + start[:, None]
    return np.clip(lo, 0, limit), np.clip(hi, 0, limit)


def edges(rois, H, W, PH, PW, scale, pad):
    sw, sh, ew, eh, rw, rh = window(rois, scale, pad)
    h0, h1 = bin_edges(sh, rh, PH, H)
    w0, w1 = bin_edges(sw, rw, PW, W)
    return h0, h1, w0, w1, rw, rh


def empty_bins(rois, H, W, PH, PW, scale, pad):
    """bool R x PH x PW: the bins the reference sets to 0 without looking at the map."""
    h0, h1, w0, w1, _, _ = edges(rois, H, W, PH, PW, scale, pad)
    return (h1 <= h0)[:, :, None] | (w1 <= w0)[:, None, :]


ROW_MAXP, ROW_SPAN, ROW_FLIGHT = 16, 128, 6        # roipool.hip: kMaxP, kMaxSpan, kRowsInFlight


def row_census(rois, H, W, PH, PW, scale, pad):
    """The branches of roipool_rows_kernel one window of every ROI takes: a set of names."""
    assert PH <= ROW_MAXP and PW <= ROW_MAXP
    h0, h1, w0, w1, _, _ = edges(rois, H, W, PH, PW, scale, pad)
    hit = set()
    for r in range(len(h0)):
        x_lo, x_hi = w0[r, 0], w1[r, -1]
        span = x_hi - x_lo
        if span <= 0:
            hit.add("span<=0")
            continue
        Wp = 8
        while Wp < min(span, ROW_SPAN):
            Wp <<= 1
        hit.add(f"Wp={Wp}")
        hit.add(f"xper={Wp // min(Wp, 64)}")
        nseg = -(-span // ROW_SPAN)
        hit.add(f"segments={min(nseg, 3)}")
        tall = int((h1[r] - h0[r]).max())
        if tall <= 0:
            hit.add("span>0,no_rows")
        if tall > ROW_FLIGHT:
            hit.add(f"tail_rem={(tall - ROW_FLIGHT) % 4}")
            if tall - ROW_FLIGHT > 4:
                hit.add("tail_iters>=2")
        nonempty = w1[r] > w0[r]
        for k in range(1, nseg):
            b = x_lo + k * ROW_SPAN
            if ((w0[r] < b) & (w1[r] > b)).any():
                hit.add("bin_straddles_segment")
            if (nonempty & (w0[r] >= b)).any():
                hit.add("bin_in_later_segment")
        if (nonempty & (w1[r] - w0[r] > 4)).any():
            hit.add("bin_wider_than_4")
    return hit


def pair_census(rois, H, W, PH, PW, scale, pad_a, pad_b):
    """roipool_rows_kernel<2>: how the two windows of a ROI differ in slot width and segment count."""
    hit = set()
    wide_pad, own_pad = max(pad_a, pad_b), min(pad_a, pad_b)
    for r in range(len(rois)):
        a = row_census(rois[r:r + 1], H, W, PH, PW, scale, wide_pad)
        b = row_census(rois[r:r + 1], H, W, PH, PW, scale, own_pad)
        wa = [int(t[3:]) for t in a if t.startswith("Wp=")]; wb = [int(t[3:]) for t in b if t.startswith("Wp=")]
        sa = [int(t[9:]) for t in a if t.startswith("segments=")]; sb = [int(t[9:]) for t in b if t.startswith("segments=")]
        if wa and wb and wa[0] > wb[0]:
            hit.add("context_slot_wider")
        if sa and sb and sa[0] > sb[0]:
            hit.add("context_more_segments")
        if ("span<=0" in a) != ("span<=0" in b):
            hit.add("one_window_outside")
    return hit


def fused_census(rois, H, W, scale, pad):
    """roipool_wino33_kernel (7 x 7 bins) on one window of every ROI: per non-empty bin the level k, the window's `wide` flag and
    whether the extra-squares loop runs; per empty bin the side of the map it fell off."""
    h0, h1, w0, w1, rw, rh = edges(rois, H, W, 7, 7, scale, pad)
    hit = set()
    for r in range(len(h0)):
        wide = bool(rw[r] >= rh[r])
        for ph in range(7):
            h = int(h1[r, ph] - h0[r, ph])
            for pw in range(7):
                w = int(w1[r, pw] - w0[r, pw])
                if h <= 0 or w <= 0:
                    if w <= 0:
                        hit.add("empty_left" if w1[r, pw] == 0 else "empty_right" if w0[r, pw] == W else "empty_inside")
                    if h <= 0:
                        hit.add("empty_top" if h1[r, ph] == 0 else "empty_bottom" if h0[r, ph] == H else "empty_inside")
                    continue
                k = min(3, int(np.log2(min(h, w))))
                s = 1 << k
                across, along = (h, w) if wide else (w, h)
                hit.add(f"k={k},wide={int(wide)}")
                if across > 2 * s or along > 4 * s:
                    hit.add(f"extra_squares,wide={int(wide)}")
    return hit


# ------------------------------------------------------------------------------------------------ the case lists
SCALES = (1 / 16, 1 / 4, 1.0)
PADS = (0.0, 0.5, 1.0)
ROW_SIZES = [(1, 1), (1, 16), (16, 1), (16, 16), (3, 5), (6, 7), (7, 7), (13, 2)]       # PH % 4 in {0,1,2,3}; 256 bins; chan_per_block 4 / capped by C
ROW_CHANNELS = (1, 5, 24, 128, 200)       # a partial last group, the C % 128 == 0 geometry, more channels than one round of slots
PERBIN_SIZES = [(17, 3), (3, 20), (17, 17)]
PERBIN_CHANNELS = (5, 128)
ALIGN_SIZES = [(1, 1), (7, 7), (4, 6), (15, 15), (17, 3)]
ALIGN_CHANNELS = (1, 5, 24, 128)

ROW_BRANCHES = ([f"Wp={w}" for w in (8, 16, 32, 64, 128)] + ["xper=1", "xper=2", "segments=1", "segments=2", "segments=3",
                "bin_straddles_segment", "bin_in_later_segment", "span<=0", "span>0,no_rows", "bin_wider_than_4",
                "tail_rem=0", "tail_rem=1", "tail_rem=2", "tail_rem=3", "tail_iters>=2"])
PAIR_BRANCHES = ["context_slot_wider", "context_more_segments", "one_window_outside"]
FUSED_BRANCHES = ([f"k={k},wide={w}" for k in range(4) for w in (0, 1)] + ["extra_squares,wide=0", "extra_squares,wide=1",
                  "empty_left", "empty_right", "empty_top", "empty_bottom"])


def row_cases():
    """[(tag, map shape, rois, PH, PW, scale, pad)]: what tests/test_gpu_roi_layers.py runs through the row kernel.  The small map
    takes every pooled size at every scale and pad; the wide and the tall map the sizes that reach their branches."""
    out = []
    for PH, PW in ROW_SIZES:
        for si, scale in enumerate(SCALES):
            for pi, pad in enumerate(PADS):
                out.append((f"std_{PH}x{PW}_s{si}_p{pi}", "std", std_rois(*STD_HW, 2, scale, seed=si), PH, PW, scale, pad))
    for PH, PW in [(1, 1), (3, 5), (7, 7), (16, 16)]:
        for scale, pad in [(1.0, 0.0), (0.25, 0.5 if PH <= WIDE_SHAPE[2] else 0.0)]:      # (16 bin rows over a padded window of a 12-row map: mostly empty)
            out.append((f"wide_{PH}x{PW}_s{scale}_p{pad}", "wide", wide_rois(scale), PH, PW, scale, pad))
    for PH, PW in [(1, 1), (3, 5), (6, 7), (7, 7)]:
        for scale, pad in [(1.0, 0.0), (0.25, 0.5)]:
            out.append((f"tall_{PH}x{PW}_s{scale}_p{pad}", "tall", tall_rois(scale), PH, PW, scale, pad))
    return out


PAIR_SIZES = [(1, 16), (3, 5), (7, 7), (16, 16), (17, 7)]       # (17, 7): the two-launch fallback
def pair_pads(kind):
    """(pad_a, pad_b): both orders, two non-zero pads, equal pads.  (Pad 1 on the 12-row wide map leaves more than half of the bins
    outside: 0.5 there.)"""
    return [(0.5, 0.0), (0.0, 0.5), (0.5 if kind == "wide" else 1.0, 0.25), (0.25, 0.25)]


def pair_sets(PH):
    """[(map, rois, scale, C)] of the pair op's cases at pooled height PH (the wide and the tall map up to 7 bin rows)."""
    sets = [("std", std_rois(*STD_HW, 2, 0.25), 0.25, 5), ("std", std_rois(*STD_HW, 2, 1.0, seed=2), 1.0, 24)]
    if PH <= 7:
        sets += [("wide", wide_rois(1.0), 1.0, 8), ("tall", tall_rois(0.25), 0.25, 8)]
    return sets


def case_shape(kind, C):
    return std_shape(C) if kind == "std" else WIDE_SHAPE if kind == "wide" else TALL_SHAPE


def fused_rois(H8, W8, batch, R, scale=0.125):
    """The first R ROIs of one list for the fused pooling + transform on a stride-8 map of H8 x W8 (at least 20 x 28).  From R = 8
    on the census (fused_census over the windows of pad 0 and 0.25) shows every branch of FUSED_BRANCHES."""
    # [x0, y0, width, height] in cells.  The first ten are chosen by bin size (7 x 7 bins): bins of >= 8, 4..7, 2..3 and 1 cells with the
    # window wider than tall and taller than wide (levels 3 .. 0), then one-cell-thin bins 8 cells long (the extra-squares loop, both
    # ways); the two largest hang over every side of the map (empty bins left, right, top and bottom).
    core = [(-10, -20, 60, 56), (-16, -12, 56, 60), (4, -3, 30, 28), (-3, 2, 28, 30), (9, 3, 15, 14), (3, 5, 14, 15), (20, 9, 7, 7),
            (11, 12, 7, 8), (-8, 6, 56, 7), (5, -16, 7, 56)]
    more = [(2.5, 1.5, 8, 5), (12, 4, -6, 6), (0, 0, W8, H8),                    # .5 edges, x2 < x1, the whole map
            (1, 1, 1, 1), (3, 2, 3, 2), (2, 3, 2, 3), (W8 - 9, 3, 14, 7), (3, H8 - 9, 7, 14), (-20, -20, W8 + 40, H8 + 40),
            (0, 4, W8, 3), (4, 0, 3, H8), (6, 6, 35, 3), (6, -4, 3, 35), (7, 7, 16, 16), (1, 2, 33, 18)]
    f = [(x0, y0, x0 + wd - 1, y0 + ht - 1) for x0, y0, wd, ht in core + more]
    out = _rows(f, batch)
    out[:, 1:] /= scale
    out = np.concatenate([out.astype(np.float32), std_rois(H8, W8, batch, scale, n_random=8, seed=R)])
    assert len(out) >= R, (len(out), R)
    return np.ascontiguousarray(out[:R])


# ------------------------------------------------------------------------------------------------ the CPU sweep and its recorded subset
SWEEP_SCALES = (1 / 16, 1 / 8, 1 / 4, 1 / 2, 1.0)
SWEEP_PADS = (0.0, 1 / 8, 1 / 4, 1 / 2, 1.0)
SWEEP_C = 3


def sweep_sizes():
    """Pooled sizes: every height 1 .. 20 with three widths that walk through 1 .. 20, and the pairs around the row kernel's limit
    (15 | 16 | 17) and at the ends, both ways round."""
    s = {(ph, 1 + (ph * k) % 20) for ph in range(1, 21) for k in (3, 7, 11)}
    for a, b in [(15, 15), (15, 16), (16, 16), (16, 17), (17, 17), (15, 17), (1, 20), (1, 1), (20, 20), (7, 7), (1, 16), (1, 17)]:
        s |= {(a, b), (b, a)}
    assert {w for _, w in s} >= set(range(1, 21))
    return sorted(s)


GOLDEN_D_ROIS = 31                                       # the hand rows and 8 random ones
GOLDEN_D_POOL = [(7, 7), (3, 5), (17, 3)]                # x GOLDEN_D_COMBOS x (relu, special)
GOLDEN_D_ALIGN = [(7, 7), (4, 6)]                        # x GOLDEN_D_COMBOS x (plain, special)
GOLDEN_D_COMBOS = [(1 / 16, 0.5), (1.0, 0.0)]            # (scale, pad)


def golden_d_cases():
    """[(key, op, map kind, PH, PW, scale, pad)]: what tests/golden/make_golden_d.py records from the reference; maps of SWEEP_C = 3
    channels, golden_d_rois(scale)."""
    out = []
    for op, sizes, kinds in (("roipool", GOLDEN_D_POOL, ("relu", "special")), ("roialign", GOLDEN_D_ALIGN, ("plain", "special"))):
        for PH, PW in sizes:
            for ci, (scale, pad) in enumerate(GOLDEN_D_COMBOS):
                for kind in kinds:
                    out.append((f"{op}_{PH}x{PW}_c{ci}_{kind}", op, kind, PH, PW, scale, pad))
    return out


def golden_d_rois(scale):
    return std_rois(*STD_HW, 2, scale, n_random=GOLDEN_D_ROIS - 23)


# ------------------------------------------------------------------------------------------------ DecodeBBox
DECODE_PARAMS = {                      # name -> (mean, std)
    "zoo_car": ((0, 0, 0, 0), (0.1, 0.1, 0.2, 0.2)),
    "zoo_ped": ((0, 0, 0, 0), (0.1, 0.1, 0.1, 0.1)),
    "zoo_cyc": ((0, 0, 0, 0), (0.2, 0.2, 0.3, 0.3)),
    "identity": ((0, 0, 0, 0), (1, 1, 1, 1)),
    "mean": ((0.1, -0.1, 0.05, -0.2), (0.2, 0.2, 0.3, 0.3)),
}
DECODE_REFUSED_STD = [(0, 1, 1, 1), (1, 1, -0.5, 1), (1, 1, 1, float("nan")), (1, -0.0, 1, 1)]
DECODE_ROWS = (1, 255, 256, 257)


def decode_inputs(R, seed=0):
    """bbox (R, 8) and prior (R, 5): random rows, then -- where R allows -- exponents across (-104, 100), NaN / inf rows and
    inverted priors.  With std 1 the exponent is the bbox value itself."""
    rng = np.random.default_rng(8100 + R + seed)
    x1 = rng.uniform(-50, 1800, R); y1 = rng.uniform(-50, 500, R)
    prior = np.stack([rng.integers(0, 2, R), x1, y1, x1 + rng.uniform(0, 600, R), y1 + rng.uniform(0, 400, R)], 1).astype(np.float32)
    bbox = (rng.standard_normal((R, 8)) * 2).astype(np.float32)
    if R >= 64:
        n = 24
        bbox[8:8 + n, 6] = np.linspace(-103.9, 99.9, n); bbox[8:8 + n, 7] = np.linspace(99.9, -103.9, n)
        bbox[40, 4:] = [np.nan, 0, 0, 0]; bbox[41, 4:] = [0, 0, np.nan, 0]; bbox[42, 4:] = [np.inf, 0, 0, -np.inf]
        bbox[43, 4:] = [0, -np.inf, np.inf, 0]; bbox[44, 4:] = [3e38, -3e38, 0, 0]
        prior[48:52, 3] = prior[48:52, 1] - 30; prior[52:56, 4] = prior[52:56, 2] - 1            # inverted priors (negative and zero sizes)
    return bbox, prior


def decode_sweep(n_lin=1 << 17, seed=0):
    """R = 2^18 rows, std 1, mean 0: bw covers (-87, 87) linearly (n_lin rows) and at random (the rest), bh the same reversed;
    prior widths 1, 37.5 and 1024 in turn."""
    R = 1 << 18
    rng = np.random.default_rng(8200 + seed)
    e = np.concatenate([np.linspace(-86.999, 86.999, n_lin), rng.uniform(-86.999, 86.999, R - n_lin)]).astype(np.float32)
    assert np.abs(e).max() < 87
    bbox = np.zeros((R, 8), np.float32)
    bbox[:, 4] = rng.standard_normal(R); bbox[:, 5] = rng.standard_normal(R)
    bbox[:, 6] = e; bbox[:, 7] = e[::-1]
    wd = np.array([1, 37.5, 1024], np.float32)[np.arange(R) % 3]
    x1 = rng.uniform(0, 500, R).astype(np.float32); y1 = rng.uniform(0, 300, R).astype(np.float32)
    prior = np.stack([np.zeros(R, np.float32), x1, y1, x1 + wd - 1, y1 + wd[::-1] - 1], 1).astype(np.float32)
    return bbox, prior


def decode_beyond(seed=0):
    """Exponents with 87 <= |x| <= 110 (std 1, mean 0), where expf_libm promises the class of the result only.  The prior is one
    pixel wide and high, so that for 87 <= x < 88.72 (expf finite, ~1e38) the decoded width IS expf(x) and its bits show in the
    output; the first half of the rows covers that range densely.  (For x <= -87 the width is below 1e-37 and vanishes in the
    sums: only the class can be observed.)"""
    R = 4096
    rng = np.random.default_rng(8300 + seed)
    mag = np.concatenate([np.linspace(87, 88.72, R // 2), np.linspace(88.72, 110, R // 4), rng.uniform(87, 110, R // 4)])
    e = mag.astype(np.float32)
    bbox = np.zeros((R, 8), np.float32)
    bbox[:, 6] = e; bbox[:, 7] = -e
    bbox[1::2, 6:8] = bbox[1::2, 7:5:-1]            # odd rows: the height takes the positive exponent
    prior = np.tile(np.array([0, 10, 20, 10, 20], np.float32), (R, 1))
    return bbox, prior
