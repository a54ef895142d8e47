"""The ROIAlign head in one pass on the GPU: mscnn_roialign_ave_pair_fwd_f32 / mscnn_roialign_ave_fwd_f32 bit for bit against the oracle's
roialign -> pool2d(AVE 2x2 / stride 1) -> concat_channels and against the device's own three-op chain, their buffer contract between
guard bands, and the Net-level switch on the reduced WiderFace cascade: every blob of a forward with the switch on -- the twelve the
fused heads did not write included -- equals the switch-off net's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from mscnn_amd import net as mnet, synth, zoo   # noqa: E402
from tests import guarded                       # noqa: E402


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X: torch.cuda.is_available() is False")
    from mscnn_amd import hipapi
    hipapi.lib()
    return hipapi


# name -> (PH, PW, scale, pad_a, pad_b), C, feature map, R, windows swapped (window b at channel offset 0)
CASES = {
    "ragged_last_group_two_images": ((5, 5, 0.125, 0.0, 0.25), 24, (2, 24, 20, 24), 61, False),
    "context_first_non_square_bins": ((4, 6, 0.25, 0.5, 0.0), 16, (2, 16, 20, 24), 61, True),
    "groups_of_16_channels": ((7, 7, 0.125, 0.0, 0.25), 128, (1, 128, 9, 12), 5, False),
    "smallest": ((1, 1, 0.125, 0.0, 0.25), 1, (1, 1, 9, 12), 1, False),
}


def make_rois(rng, R, N, H, W, scale):
    """Fractional ROIs in image coordinates, mostly on the map; rows 0 .. 8 by hand where R allows (the whole map comes first so that
    the one-ROI case samples something)."""
    ih, iw = H / scale, W / scale
    x1 = rng.uniform(-0.1 * iw, 0.8 * iw, R); y1 = rng.uniform(-0.1 * ih, 0.8 * ih, R)
    w = rng.uniform(3.0, 0.6 * iw, R); h = rng.uniform(3.0, 0.6 * ih, R)
    rois = np.stack([rng.integers(0, N, R).astype(np.float64), x1, y1, x1 + w, y1 + h], 1)
    hand = [
        [0, 0, 0, iw - 1, ih - 1],                               # the whole map
        [N - 1, 0.3 * iw + 0.37, 0.0, 0.7 * iw + 0.11, ih],      # pad 0: first grid row exactly on -0.5, last exactly on H - 0.5
        [N - 1, -0.3 * iw, 0.3 * ih + 0.25, 0.3 * iw, 0.6 * ih],   # straddles the left border
        [0, 0.7 * iw + 0.5, 0.3 * ih, 1.3 * iw, 0.6 * ih],       # the right border
        [0, 0.3 * iw, -0.3 * ih, 0.6 * iw + 0.75, 0.3 * ih],     # the top border
        [N - 1, 0.3 * iw, 0.7 * ih, 0.6 * iw, 1.3 * ih + 0.125],   # the bottom border
        [0, -5 * iw, -5 * ih, -4 * iw, -4 * ih],                 # far off the map: all zeros
        [0, 0.6 * iw, 0.2 * ih, 0.6 * iw - 9.5, 0.5 * ih],       # x2 < x1
    ]
    k = min(R, len(hand))
    rois[:k] = hand[:k]
    return rois.astype(np.float32)


_INPUTS = {}


def case_inputs(name, orc):
    """(feat, rois, oracle result with window a's channels first then b's or the other way round, offsets) -- computed once per case."""
    if name not in _INPUTS:
        (ph, pw, scale, pad_a, pad_b), C_, shape, R, swapped = CASES[name]
        rng = np.random.default_rng(sum(map(ord, name)))
        feat = rng.standard_normal(shape).astype(np.float32)
        rois = make_rois(rng, R, shape[0], shape[2], shape[3], scale)
        win = {p: orc.pool2d(orc.roialign(feat, rois, ph, pw, scale, p), (2, 2), (0, 0), (1, 1), "AVE") for p in (pad_a, pad_b)}
        off_a, off_b = (C_, 0) if swapped else (0, C_)
        ref = orc.concat_channels([win[pad_b], win[pad_a]] if swapped else [win[pad_a], win[pad_b]])
        assert ref.shape == (R, 2 * C_, ph, pw) and np.isfinite(ref).all()
        for a in (feat, rois, ref):
            a.setflags(write=False)
        _INPUTS[name] = (feat, rois, ref, win, off_a, off_b)
    return _INPUTS[name]


@pytest.mark.parametrize("name", list(CASES))
def test_inputs_exercise_what_they_claim(orc, name):
    (ph, pw, scale, pad_a, pad_b), C_, shape, R, swapped = CASES[name]
    feat, rois, ref, win, _, _ = case_inputs(name, orc)
    zeros = float((ref == 0).mean())
    print(f"{name}: {zeros:.3f} of the reference outputs are exactly zero")
    assert zeros <= 0.5                                 # a kernel that writes zeros cannot pass
    if R >= 8:
        assert not ref[6].any()                         # far off the map
        for r in (2, 3, 4, 5):                          # border ROIs: outside samples (0) averaged with inside ones
            assert (ref[r] == 0).any() and (ref[r] != 0).any(), r
        # the ROI whose pad-0 grid rows land exactly on -0.5 and on H - 0.5: both rows are inside by the reference's test
        if shape[2] % ph == 0:
            grid = orc.roialign(feat, rois[1:2], ph, pw, scale, 0.0)
            assert (grid[0, :, 0, :] != 0).all() and (grid[0, :, ph, :] != 0).all()


@pytest.mark.parametrize("name", list(CASES))
def test_pair_op_equals_the_oracle_composition(hip, orc, name):
    (ph, pw, scale, pad_a, pad_b), C_, shape, R, swapped = CASES[name]
    feat, rois, ref, _, off_a, off_b = case_inputs(name, orc)
    y = hip.roialign_ave_pair(torch.from_numpy(feat.copy()).cuda(), torch.from_numpy(rois.copy()).cuda(), ph, pw, scale, pad_a, pad_b,
                              c_offset_a=off_a, c_offset_b=off_b)
    assert tuple(y.shape) == ref.shape
    assert np.array_equal(y.cpu().numpy(), ref)


@pytest.mark.parametrize("name", list(CASES))
def test_single_op_gives_each_window(hip, orc, name):
    (ph, pw, scale, pad_a, pad_b), C_, shape, R, swapped = CASES[name]
    feat, rois, ref, win, off_a, off_b = case_inputs(name, orc)
    fd, rd = torch.from_numpy(feat.copy()).cuda(), torch.from_numpy(rois.copy()).cuda()
    for pad in (pad_a, pad_b):
        assert np.array_equal(hip.roialign_ave(fd, rd, ph, pw, scale, pad).cpu().numpy(), win[pad]), pad
    # two single calls into the windows of one output = the pair op
    out = torch.full(ref.shape, float("nan"), dtype=torch.float32, device="cuda")
    hip.roialign_ave(fd, rd, ph, pw, scale, pad_a, out=out, c_total=2 * C_, c_offset=off_a)
    hip.roialign_ave(fd, rd, ph, pw, scale, pad_b, out=out, c_total=2 * C_, c_offset=off_b)
    assert np.array_equal(out.cpu().numpy(), ref)


@pytest.mark.parametrize("name", list(CASES))
def test_both_ops_equal_the_device_chain(hip, orc, name):
    (ph, pw, scale, pad_a, pad_b), C_, shape, R, swapped = CASES[name]
    feat, rois, _, _, off_a, off_b = case_inputs(name, orc)
    fd, rd = torch.from_numpy(feat.copy()).cuda(), torch.from_numpy(rois.copy()).cuda()
    pooled = {p: hip.pool2d(hip.roialign(fd, rd, ph, pw, scale, p), (2, 2), (0, 0), (1, 1), "AVE") for p in (pad_a, pad_b)}
    chain = hip.concat_channels([pooled[pad_b], pooled[pad_a]] if swapped else [pooled[pad_a], pooled[pad_b]])
    y = hip.roialign_ave_pair(fd, rd, ph, pw, scale, pad_a, pad_b, c_offset_a=off_a, c_offset_b=off_b)
    assert torch.equal(y, chain)
    for pad in (pad_a, pad_b):
        assert torch.equal(hip.roialign_ave(fd, rd, ph, pw, scale, pad), pooled[pad])


@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "bases_4_bytes_off"])
def test_buffer_contract(hip, orc, lead):
    """C_total = 2C + 8: the eight channels between the windows and both guard bands keep their poison; feat / rois between NaN guards
    are read inside their bounds only and are not written; with lead = 1 every base lies 4 bytes past a 512-byte boundary."""
    name = "ragged_last_group_two_images"
    (ph, pw, scale, pad_a, pad_b), C_, shape, R, _ = CASES[name]
    feat, rois, ref, win, _, _ = case_inputs(name, orc)
    arena = guarded.Arena("cuda")
    fd, rd = arena.input(feat, np.nan), arena.input(rois, np.nan)
    c_total = 2 * C_ + 8
    out = arena.alloc((R, c_total, ph, pw))
    one = arena.alloc((R, c_total, ph, pw))
    if lead:
        fd, rd, out, one = (arena.offset_view(t, lead) for t in (fd, rd, out, one))
        assert all(t.data_ptr() % 16 == 4 for t in (fd, rd, out, one))
    hip.roialign_ave_pair(fd, rd, ph, pw, scale, pad_a, pad_b, out=out, c_total=c_total, c_offset_a=0, c_offset_b=C_ + 8)
    hip.roialign_ave(fd, rd, ph, pw, scale, pad_b, out=one, c_total=c_total, c_offset=C_ + 8)
    torch.cuda.synchronize()
    arena.check()
    got = out.cpu().numpy()
    assert np.array_equal(got[:, :C_], win[pad_a]) and np.array_equal(got[:, C_ + 8:], win[pad_b])
    assert guarded.all_poison(out[:, C_:C_ + 8].contiguous())
    assert np.array_equal(one.cpu().numpy()[:, C_ + 8:], win[pad_b])
    assert guarded.all_poison(one[:, :C_ + 8].contiguous())


# ---------------------------------------------------------------------------------------------------------------- Net level
MODEL, SIZE = "widerface/cascade-mscnn-12s-align", dict(height=160, width=192, max_nms_num=150)
ORG_HW = (600, 720)
OUTPUT_3RD = ("output_bbox_3rd", "cls_prob_3rd_avg", "proposals_3rd")


def frames(batch, seed):
    return np.concatenate([synth.frame(SIZE["height"], SIZE["width"], seed=seed + 100 * b, org_hw=ORG_HW) for b in range(batch)], 0)


def new_net(batch, on):
    n = mnet.Net(prototxt_text=zoo.prototxt(MODEL, batch=batch, **SIZE))
    synth.load_into(n, "mid")
    if on:
        n.set_roialign_one_pass(True)
    return n


def run(n, x, start=0, end=-1):
    if x is not None:
        n.set_blob("data", x)
    n.forward(start, end)


def same_blobs(a, b, what):
    for name in a.blob_names:
        assert a.blob_shape(name) == b.blob_shape(name), (what, name)
        assert np.array_equal(a.get_blob(name), b.get_blob(name)), (what, name)


def final_stage(n, batch):
    H, W = SIZE["height"], SIZE["width"]
    kw = dict(ratios=(H / float(ORG_HW[0]), W / float(ORG_HW[1])), org_hw=ORG_HW)
    if batch == 1:
        dets, ids, R = n.detect_cascade(*OUTPUT_3RD, cls_id=2, det_thr=0.0, **kw)
        return [dets.tobytes(), ids.tobytes(), R]
    per_image, counts = n.detect_cascade_multi([kw] * batch, [OUTPUT_3RD], [2])
    return [[(d.tobytes(), i.tobytes()) for d, i in img[0]] for img in per_image] + [counts]


_NETS = {}


def nets(batch):
    """(switch-off net, switch-on net) with the same weights, each after one whole forward of the same frame(s)."""
    if batch not in _NETS:
        x = frames(batch, 1701)
        off, on = new_net(batch, False), new_net(batch, True)
        run(off, x); run(on, x)
        _NETS[batch] = (off, on)
    return _NETS[batch]


@pytest.mark.parametrize("batch", [1, 2])
def test_net_one_pass_keeps_every_blob(hip, batch):
    off, on = nets(batch)
    heads = on.roialign_pairs()
    assert len(heads) == 3 and off.roialign_pairs() == heads
    assert [on.layer_kernel(i) for i in heads] == ["roialign_ave_pair"] * 3
    assert [off.layer_kernel(i) for i in heads] == [""] * 3
    assert on.blob_shape("proposals")[0] > 8
    # the Concat's tops first (written by the one-pass launch), then every blob: the twelve the fused forward did not write are made
    # on demand by the very layers the switch-off net ran
    for sfx in ("", "_2nd", "_3rd"):
        assert np.array_equal(on.get_blob("roi_pool" + sfx), off.get_blob("roi_pool" + sfx)), sfx
        assert on.get_blob("roi_pool" + sfx).any()
    same_blobs(on, off, "whole forward")
    assert [on.layer_kernel(i) for i in heads] == ["roialign_ave_pair"] * 3      # reading blobs does not change the report
    assert final_stage(on, batch) == final_stage(off, batch)


@pytest.mark.parametrize("batch", [1, 2])
def test_net_switch_toggled_across_forwards(hip, batch):
    """on -> off -> on, a new frame each: every forward equals a net's that never had the switch on -- the module's switch-off net for
    the first two (one reference forward each), a net built for the purpose for the last."""
    off, n = nets(batch)
    heads = n.roialign_pairs()
    for k, on in enumerate((True, False, True)):
        x = frames(batch, 40 + k)
        n.set_roialign_one_pass(on)
        run(n, x)
        assert [n.layer_kernel(i) for i in heads] == (["roialign_ave_pair"] * 3 if on else [""] * 3)
        fresh = off if k < 2 else new_net(batch, False)
        run(fresh, x)
        same_blobs(n, fresh, f"forward {k}, switch {'on' if on else 'off'}")
        assert final_stage(n, batch) == final_stage(fresh, batch)


@pytest.mark.parametrize("batch", [1, 2])
def test_net_partial_forward_from_inside_a_head(hip, batch):
    """A range that starts at roi_pool_org holds four of the first head's five layers: they run stand-alone, from a roi_grid_org that is
    written first (the whole forward before it ran the head in one pass); the later heads lie inside the range and run in one pass."""
    off, on = nets(batch)
    heads = on.roialign_pairs()
    x = frames(batch, 1701)
    for n in (off, on):
        run(n, x)
    start = on.layer_names.index("roi_pool_org")
    assert heads[0] < start < on.layer_names.index("roi_pool")
    for n in (off, on):
        run(n, None, start, len(n.layer_names) - 1)
    assert [on.layer_kernel(i) for i in heads[1:]] == ["roialign_ave_pair"] * 2
    same_blobs(on, off, "partial forward")
    assert final_stage(on, batch) == final_stage(off, batch)
    # a range that ends inside a head: stand-alone as well, and the blobs behind the range still read as the frame before
    end = on.layer_names.index("roi_grid_ctx_2nd")
    for n in (off, on):
        run(n, frames(batch, 99), 0, end)
    assert on.layer_kernel(heads[0]) == "roialign_ave_pair" and on.layer_kernel(heads[1]) == ""
    same_blobs(on, off, "range that ends inside the second head")
