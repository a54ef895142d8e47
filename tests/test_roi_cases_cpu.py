"""CPU census of tests/roi_cases.py: the geometry restatement is held to the oracle, and the case lists are shown to reach every
kernel branch that tests/test_gpu_roi_layers.py is meant to run (the branch names are roi_cases.ROW_BRANCHES / PAIR_BRANCHES /
FUSED_BRANCHES).  Run with -s to read, per case, the branches it hits."""
import numpy as np
import pytest

import roi_cases as rc


def test_roundf_is_half_away_from_zero():
    x = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.49999997, -0.49999997, 8388609.0, -3.0, 0.0], np.float32)
    assert rc.roundf(x).tolist() == [1, -1, 2, -2, 3, -3, 0, 0, 8388609, -3, 0]


@pytest.mark.parametrize("pad", rc.PADS)
@pytest.mark.parametrize("scale", rc.SCALES)
def test_restatement_empty_bins_match_the_oracle(orc, scale, pad):
    """On a strictly positive map a bin is empty in the restatement exactly when the oracle's output is 0 -- every pooled size of the
    row and per-bin cases, every ROI set."""
    sets = [(rc.std_shape(3), rc.std_rois(*rc.STD_HW, 2, scale)), (rc.WIDE_SHAPE, rc.wide_rois(scale)), (rc.TALL_SHAPE, rc.tall_rois(scale)),
            ((2, 3, 24, 40), rc.fused_rois(24, 40, 2, 45, scale))]
    for shape, rois in sets:
        feat = rc.positive_map((shape[0], 2) + shape[2:])
        for PH, PW in rc.ROW_SIZES + rc.PERBIN_SIZES:
            y = orc.roipool(feat, rois, PH, PW, scale, pad)
            empty = rc.empty_bins(rois, shape[2], shape[3], PH, PW, scale, pad)
            assert np.array_equal(y == 0, np.broadcast_to(empty[:, None], y.shape)), (shape, PH, PW, scale, pad)


def test_half_edges_are_exact_halves():
    """The hand rows meant to land on .5 before roundf do (pad 0: the product with the scale is exact for these power-of-two scales)."""
    for scale in rc.SCALES:
        r = rc.hand_rois(*rc.STD_HW, 2, scale).astype(np.float32)
        v = r[11:14, 1:] * np.float32(scale)
        assert np.all(np.abs(v - np.floor(v)) == 0.5), (scale, v)
        assert (v < 0).any() and (v > 0).any()


def test_row_kernel_cases_reach_every_branch():
    seen = set()
    for tag, kind, rois, PH, PW, scale, pad in rc.row_cases():
        N, C, H, W = rc.case_shape(kind, 8)
        hit = rc.row_census(rois, H, W, PH, PW, scale, pad)
        print(f"{tag}: {' '.join(sorted(hit))}")
        seen |= hit
        empty = rc.empty_bins(rois, H, W, PH, PW, scale, pad)
        assert empty.mean() <= 0.5, (tag, empty.mean())          # no case is mostly zeros
    missing = [b for b in rc.ROW_BRANCHES if b not in seen]
    assert not missing, missing
    assert {ph % 4 for ph, _ in rc.ROW_SIZES} == {0, 1, 2, 3} and (16, 16) in rc.ROW_SIZES
    # chan_per_block = 1024 / bins: 4 at 256 bins, capped by C at 1 x 1; C % 128 == 0 -> 16; 200 channels > one round of 32 slots
    assert 1024 // 256 == 4 and 128 in rc.ROW_CHANNELS and max(rc.ROW_CHANNELS) > 128 and 5 in rc.ROW_CHANNELS


def test_outside_rows_are_the_only_all_empty_ones():
    """The hand rows that lie outside are wholly empty (so the `more than half zeros` rule above excuses only them)."""
    for scale in rc.SCALES:
        rois = rc.std_rois(*rc.STD_HW, 2, scale)
        e = rc.empty_bins(rois, *rc.STD_HW, 7, 7, scale, 0.0).reshape(len(rois), -1)
        assert e[:6].all() and not e[6].any()
        assert not e[8:11].all(1).any()                 # inverted ROIs are NOT empty: the window is at least one cell (max(.., 1))


def test_pair_cases_reach_every_branch():
    """The pair op's own case list: somewhere the context window takes a wider slot and more column segments than the ROI's own
    window, and somewhere only one of the two windows lies outside the map; (17, 7) is beyond the row kernel (two launches)."""
    seen = set()
    for PH, PW in rc.PAIR_SIZES:
        if PH > rc.ROW_MAXP or PW > rc.ROW_MAXP:
            continue
        for kind, rois, scale, Cc in rc.pair_sets(PH):
            N, C, H, W = rc.case_shape(kind, Cc)
            for pad_a, pad_b in rc.pair_pads(kind):
                for pad in (pad_a, pad_b):
                    assert rc.empty_bins(rois, H, W, PH, PW, scale, pad).mean() <= 0.5, (kind, PH, PW, scale, pad)
                hit = rc.pair_census(rois, H, W, PH, PW, scale, pad_a, pad_b)
                print(f"pair {kind} {PH}x{PW} scale {scale} pads {pad_a} / {pad_b}: {' '.join(sorted(hit))}")
                assert (pad_a != pad_b) or not hit
                seen |= hit
    missing = [b for b in rc.PAIR_BRANCHES if b not in seen]
    assert not missing, missing
    assert any(PH > rc.ROW_MAXP or PW > rc.ROW_MAXP for PH, PW in rc.PAIR_SIZES)


@pytest.mark.parametrize("H8,W8,batch,R", [(24, 40, 1, 8), (24, 40, 2, 13), (20, 28, 2, 45)])
def test_fused_cases_reach_every_branch(H8, W8, batch, R):
    """Every ROI set of the fused GPU test shows, over its two windows, every level with both values of `wide`, the extra-squares
    loop and empty bins on each side -- the 8-ROI set (the smallest plan that fuses) included."""
    rois = rc.fused_rois(H8, W8, batch, R)
    assert len(rois) == R and rois[:, 0].max() < batch
    hit = rc.fused_census(rois, H8, W8, 0.125, 0.0) | rc.fused_census(rois, H8, W8, 0.125, 0.25)
    print(f"fused {H8}x{W8} R={R}: {' '.join(sorted(hit))}")
    missing = [b for b in rc.FUSED_BRANCHES if b not in hit]
    assert not missing, missing


def test_per_bin_align_and_fused_cases_are_not_mostly_empty():
    """No case of the per-bin kernel, ROIAlign (its bins, as a measure of its grid) or the fused sets has more than half of its
    bins outside the map."""
    for PH, PW in rc.PERBIN_SIZES + rc.ALIGN_SIZES:
        for si, scale in enumerate(rc.SCALES):
            rois = rc.std_rois(*rc.STD_HW, 2, scale, seed=si)
            for pad in rc.PADS:
                assert rc.empty_bins(rois, *rc.STD_HW, PH, PW, scale, pad).mean() <= 0.5, (PH, PW, scale, pad)
    for H8, W8, batch, R in [(24, 40, 1, 8), (24, 40, 2, 13), (20, 28, 2, 45)]:
        rois = rc.fused_rois(H8, W8, batch, R)
        for pad in (0.0, 0.25):
            assert rc.empty_bins(rois, H8, W8, 7, 7, 0.125, pad).mean() <= 0.5, (R, pad)


def test_decode_inputs_cover_what_they_claim():
    bbox, prior = rc.decode_inputs(257)
    assert np.nanmin(bbox[:, 6]) < -103 and np.nanmax(bbox[:, 6][np.isfinite(bbox[:, 6])]) > 99 and np.isnan(bbox).any() and np.isinf(bbox).any()
    assert (prior[:, 3] < prior[:, 1]).any() and (prior[:, 4] < prior[:, 2]).any()
    bbox, prior = rc.decode_sweep()
    assert len(bbox) == 1 << 18 and np.abs(bbox[:, 6:]).max() < 87 and set(np.unique(prior[:, 3] - prior[:, 1] + 1)) >= {1.0}
    e = np.sort(bbox[:, 6])
    assert np.diff(e).max() < 2e-3                        # dense: no gap of (-87, 87) wider than 0.002
    bbox, _ = rc.decode_beyond()
    assert np.abs(bbox[:, 6]).min() >= 87
