"""The Net on a caller's stream (include/mscnn_net.h: mscnn_net_set_stream; mscnn_amd.net.set_stream / on_stream): a net's frame is
enqueued on the stream that is set, per host thread, when its calls are made.  Every comparison is bit for bit with the same net, or
an identically built one, on the default stream; no tolerance is introduced.  Synthetic weights, 96 x 160 frames, three deploy nets:
a plain one, a "-2x" deconvolution net and the ROIAlign cascade."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from mscnn_amd import net as mnet, synth, zoo   # noqa: E402
from tests import streams                        # noqa: E402

H, W = 96, 160
ORG_HW = (375, 1242)
PARAMS = [dict(ratios=(H / float(ORG_HW[0]), W / float(ORG_HW[1])), org_hw=ORG_HW)]
MODELS = {   # model, classes, cascade
    "car": ("kitti_car/mscnn-7s-576", [2], False),
    "ped_cyc_2x": ("kitti_ped_cyc/mscnn-7s-576-2x", [2, 3], False),
    "align_cascade": ("widerface/cascade-mscnn-12s-align", [2], True),
}


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X: torch.cuda.is_available() is False")
    from mscnn_amd import hipapi
    hipapi.lib()
    return hipapi


def new_net(key):
    n = mnet.Net(prototxt_text=zoo.prototxt(MODELS[key][0], height=H, width=W, max_nms_num=100))
    synth.load_into(n, "mid")
    return n


def frame(seed):
    return torch.from_numpy(synth.frame(H, W, seed=seed, org_hw=ORG_HW)).cuda()


def cascade_outputs(n):
    return [("output_bbox_1st", "cls_prob_1st", "proposals"), ("output_bbox_2nd", "cls_prob_2nd", "proposals_2nd"),
            ("output_bbox_3rd", "cls_prob_3rd_avg" if "cls_prob_3rd_avg" in n.blob_names else "cls_prob_3rd", "proposals_3rd")]


def subnet_blobs(n):
    """Every blob a layer from BoxOutput on writes: the ROI blobs and the prediction blobs."""
    L, _ = n.forward_rois_layers()
    names = []
    for i in range(L, len(n.layer_names)):
        names += [t for t in n.layer_tops(i) if t not in names]
    return names


def final_stage(n, key):
    """Every detection of the frame as one flat list of (dets, ids), the ROI counts, and the proposal result where the net has one."""
    _, classes, cascade = MODELS[key]
    if cascade:
        per_image, rois = n.detect_cascade_multi(PARAMS, cascade_outputs(n), classes)
        segs = [seg for img in per_image for out in img for seg in out]
    else:
        per_image, rois = n.detect_multi(PARAMS, classes)
        segs = [seg for img in per_image for seg in img]
    props = None if cascade else n.proposals_multi(PARAMS)      # (a cascade deploy restates no proposals_score: the call refuses it)
    return segs, rois, props


def after_forward(n, key):
    segs, rois, props = final_stage(n, key)
    return dict(segs=segs, rois=rois, props=props, blobs={name: n.get_blob(name) for name in subnet_blobs(n)})


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def assert_same(got, ref, what):
    assert got["rois"] == ref["rois"] and len(got["segs"]) == len(ref["segs"]), what
    for (d, i), (rd, ri) in zip(got["segs"], ref["segs"]):
        assert d.shape == rd.shape and np.array_equal(bits(d), bits(rd)) and np.array_equal(i, ri), what
    if ref["props"] is not None:
        (gp, gr), (rp, rr) = got["props"], ref["props"]
        assert gr == rr and len(gp) == len(rp), what
        for (p, rows), (wp, wrows) in zip(gp, rp):
            assert p.shape == wp.shape and np.array_equal(bits(p), bits(wp)) and np.array_equal(rows, wrows), what
    assert sorted(got["blobs"]) == sorted(ref["blobs"])
    for name, r in ref["blobs"].items():
        g = got["blobs"][name]
        assert g.shape == r.shape and np.array_equal(bits(g), bits(r)), (what, name)


@pytest.mark.parametrize("key", list(MODELS))
def test_a_frame_on_a_side_stream_equals_the_frame_on_the_default_stream(hip, key):
    """The same net, the same frame: first on the default stream, then -- the caller orders the two streams with wait_stream -- on a
    side stream behind a gate, with the input tensor holding a stale frame until a copy on the side stream replaces it, and
    overwritten again behind forward.  Every blob from BoxOutput on and every detection bit for bit.  forward waits for the ROI count
    in the middle, by design, so `busy` is asserted for the device-to-device set_blob only."""
    n = new_net(key)
    real, stale, third = frame(1701), frame(1714), frame(1727)
    assert not torch.equal(real, stale) and not torch.equal(real, third)
    n.set_blob("data", real)
    n.forward()
    ref = after_forward(n, key)
    assert sum(len(d) for d, _ in ref["segs"]) > 0, "no detection at all: the case shows nothing"
    handoff = n.handoff_state()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    buf = stale.clone()
    torch.cuda.synchronize()
    streams.calibrate(side)

    def on_side(gate_ms):
        buf.copy_(stale)
        torch.cuda.synchronize()
        with torch.cuda.stream(side), mnet.on_stream(side):
            if gate_ms:
                streams.gate(side, gate_ms)
            t0 = time.perf_counter()
            buf.copy_(real, non_blocking=True)
            n.set_blob("data", buf)
            busy = not side.query()
            ms = (time.perf_counter() - t0) * 1e3
            n.forward()
            buf.copy_(third, non_blocking=True)
            got = after_forward(n, key)
            side.synchronize()
        return busy, ms, got

    _, enqueue_ms, got = on_side(0)
    assert_same(got, ref, f"{key}: ungated side-stream frame")
    gate_ms = max(streams.GATE_FACTOR * enqueue_ms, streams.MIN_GATE_MS)
    busy, _, got = on_side(gate_ms)
    print(f"[stream] net {key}: set_blob enqueue {enqueue_ms:.3f} ms, gate {gate_ms:.2f} ms, busy {busy}")
    assert busy, f"{key}: the side stream was idle when set_blob returned (gate {gate_ms:.2f} ms)"
    assert_same(got, ref, f"{key}: gated side-stream frame")
    assert n.handoff_state() == handoff
    # back on the default stream (ordered behind the side stream, which was synchronised): the same frame again
    n.set_blob("data", real)
    n.forward()
    assert_same(after_forward(n, key), ref, f"{key}: default stream again")


def test_pipelined_detect_pairs_on_a_side_stream_equal_detect_per_frame(hip):
    """detect_begin / detect_end over three frames on the side stream (the pinned slots and their events live on the net's stream)
    against detect per frame on the default stream."""
    n = new_net("car")
    frames = [frame(1701 + 13 * i) for i in range(3)]
    kw = dict(cls_id=2, ratios=PARAMS[0]["ratios"], org_hw=ORG_HW)
    want = []
    for x in frames:
        n.set_blob("data", x)
        n.forward()
        want.append(n.detect(cap=512, **kw))
    assert sum(len(d) for d, _, _ in want) > 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = []
    with torch.cuda.stream(side), mnet.on_stream(side):
        for t, x in enumerate(frames):
            n.set_blob("data", x)
            n.forward()
            n.detect_begin(512, **kw)
            if t >= 1:
                got.append(n.detect_end(512))
        got.append(n.detect_end(512))
        side.synchronize()
    assert len(got) == 3
    for t, ((d, i, r), (wd, wi, wr)) in enumerate(zip(got, want)):
        assert r == wr and d.shape == wd.shape and np.array_equal(bits(d), bits(wd)) and np.array_equal(i, wi), t


def test_numerics_watch_on_a_side_stream(hip):
    """set_numerics_watch(1): every forward re-checks one Winograd layer behind the frame on the net's stream.  Two identically built
    nets, two frames each: the same frames and the same numerics_watch_state() on the side stream as on the default stream."""
    frames = [frame(1701), frame(1714)]

    def run(n):
        n.set_numerics_watch(1, 5e-5)
        out = []
        for x in frames:
            n.set_blob("data", x)
            n.forward()
            out.append(after_forward(n, "car"))
        return out, n.numerics_watch_state()

    want, wstate = run(new_net("car"))
    assert wstate[0] >= 1 and wstate[1] == [], wstate
    b = new_net("car")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), mnet.on_stream(side):
        got, gstate = run(b)
        side.synchronize()
    assert gstate == wstate
    for t in range(2):
        assert_same(got[t], want[t], f"watched frame {t}")


def test_tracker_on_a_side_stream(hip):
    """set_tracker with detect_tracks over three frames: the same ids and boxes on the side stream as on the default stream, each
    from a fresh tracker."""
    n = new_net("car")
    frames = [frame(1701), frame(1701), frame(1714)]      # (a repeated frame: its tracks are found again)

    def run():
        n.set_tracker(high_thr=0.1, low_thr=0.05, match_thr=0.3, match_thr_low=0.5, motion="linear", max_age=5, min_hits=1, max_tracks=64)
        out = []
        for x in frames:
            n.set_blob("data", x)
            n.forward()
            per_image, rois = n.detect_multi(PARAMS, [2])
            out.append((per_image[0][0], n.detect_tracks()[0][0]))
        n.set_tracker(None)
        return out

    want = run()
    assert any((ids > 0).any() for _, ids in want), "no detection got a track id: the case shows nothing"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), mnet.on_stream(side):
        got = run()
        side.synchronize()
    for t, (((d, i), ids), ((wd, wi), wids)) in enumerate(zip(got, want)):
        assert d.shape == wd.shape and np.array_equal(bits(d), bits(wd)) and np.array_equal(i, wi) and np.array_equal(ids, wids), t


def test_two_nets_on_two_streams_from_one_thread(hip):
    """The car net on one stream and the pedestrian / cyclist net on another, alternating from one host thread for three frames --
    their InnerProduct layers share the library's slab table, which keeps a buffer per stream.  Whole tiles are forced for the
    duration: the plane GEMM's split tiles wait inside the kernel for co-resident workgroups, which two streams sharing the device
    do not promise.  Each net's last frame is bit-identical to its serial run under the same setting; no hand-off event."""
    frames = [frame(1701 + 13 * i) for i in range(3)]
    hip.wgemm_force_whole_tiles(True)
    try:
        nets = {k: new_net(k) for k in ("car", "ped_cyc_2x")}
        want = {}
        for k, n in nets.items():
            for x in frames:
                n.set_blob("data", x)
                n.forward()
            want[k] = after_forward(n, k)
        handoff = {k: n.handoff_state() for k, n in nets.items()}
        torch.cuda.synchronize()
        s = {"car": torch.cuda.Stream(), "ped_cyc_2x": torch.cuda.Stream()}
        for x in frames:
            for k, n in nets.items():
                mnet.set_stream(s[k])
                n.set_blob("data", x)
                n.forward()
        got = {}
        for k, n in nets.items():
            mnet.set_stream(s[k])
            got[k] = after_forward(n, k)
        for st in s.values():
            st.synchronize()
        for k in nets:
            assert_same(got[k], want[k], f"{k} beside the other net")
            assert nets[k].handoff_state() == handoff[k]
    finally:
        mnet.set_stream(None)
        hip.wgemm_force_whole_tiles(False)
