"""Batched pre-processing on the GPU: mscnn_preprocess_batch_u8_f32 against the single-frame op and the oracle (bit for bit, every
slice, chunks of 32 frames included), Net.set_images with host and with device frames, set_images -> forward -> detect_multi against
the same net fed the oracle's input, the refusals (blob unchanged), and the demo driver's --batch against its batch-1 run."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from mscnn_amd import net as mnet, synth, zoo   # noqa: E402

CAP = 32          # frames per launch of preprocess.hip (kMaxImages)
NET_H, NET_W = 192, 640
# mixed sizes against 192 x 640: grows on both axes (equal scales: H first), shrinks on both (W first), grows on H and shrinks on W
# (W first), shrinks on H and grows on W (H first)
NET_ORGS = [(150, 500), (250, 900), (100, 700), (300, 480)]
CLASSES = [2, 3]


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X: torch.cuda.is_available() is False")
    from mscnn_amd import hipapi
    hipapi.lib()
    return hipapi


def rgb(h, w, seed):
    """uint8 RGB [h, w, 3]: blocky low-frequency noise, a few flat rectangles and fine noise on top (edges for the cubic taps)."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0, 255, (h // 6 + 1, w // 6 + 1, 3))
    img = np.repeat(np.repeat(base, 6, 0), 6, 1)[:h, :w]
    for _ in range(4):
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        img[y:y + int(rng.integers(1, h // 2 + 2)), x:x + int(rng.integers(1, w // 2 + 2))] = rng.uniform(0, 255, 3)
    img = img + rng.normal(0, 6, img.shape)
    return np.ascontiguousarray(np.clip(img, 0, 255).astype(np.uint8))


def h_first(org, H, W):
    return H / org[0] <= W / org[1]


def check_batch(hip, orc, orgs, H, W, mean=(104.0, 117.0, 123.0), seed=0):
    frames = [rgb(h, w, seed + 13 * i) for i, (h, w) in enumerate(orgs)]
    dev = [torch.from_numpy(f).cuda() for f in frames]
    out = hip.preprocess_batch(dev, H, W, mean_bgr=mean).cpu().numpy()
    assert out.shape == (len(frames), 3, H, W) and out.dtype == np.float32
    for b, f in enumerate(frames):
        one = hip.preprocess(dev[b], H, W, mean_bgr=mean).cpu().numpy()
        assert np.array_equal(out[b:b + 1], one), (b, orgs[b])
        assert np.array_equal(out[b:b + 1], orc.preprocess(f, H, W, mean_bgr=mean)), (b, orgs[b])


def test_preprocess_batch_of_one(hip, orc):
    check_batch(hip, orc, [(75, 248)], 96, 320)


def test_preprocess_batch_mixed_sizes_in_one_launch(hip, orc):
    H, W = 96, 320
    orgs = [(200, 700),       # shrinks on both axes (W first)
            (40, 150),        # grows on both axes (W first)
            (300, 500),       # shrinks on H, grows on W (H first) -- next to a W-first frame
            (96, 320),        # already at the target size
            (8, 900),         # extreme aspect ratios
            (700, 6),
            (97, 321)]
    assert {h_first(o, H, W) for o in orgs} == {True, False}
    check_batch(hip, orc, orgs, H, W, seed=1)
    check_batch(hip, orc, orgs[:3], H, W, mean=(100.0, 110.5, 120.0), seed=2)      # B = 3, a mean of its own


def test_preprocess_batch_above_one_launch(hip, orc):
    rng = np.random.default_rng(7)
    orgs = [(int(rng.integers(3, 48)), int(rng.integers(3, 64))) for _ in range(CAP + 3)]    # two chunks: 32 + 3
    check_batch(hip, orc, orgs, 24, 40, seed=3)


def test_preprocess_batch_refuses_bad_frames(hip):
    ok = torch.zeros((10, 12, 3), dtype=torch.uint8, device="cuda")
    for bad in (torch.zeros((10, 12, 3), dtype=torch.float32, device="cuda"), torch.zeros((10, 12, 4), dtype=torch.uint8, device="cuda"),
                torch.zeros((12, 10, 3), dtype=torch.uint8, device="cuda").transpose(0, 1)):
        with pytest.raises(hip.MscnnError):
            hip.preprocess_batch([ok, bad], 8, 8)
    with pytest.raises(hip.MscnnError, match="bad shape 0 x 12"):
        hip.preprocess_batch([ok, torch.zeros((0, 12, 3), dtype=torch.uint8, device="cuda")], 8, 8)


# ------------------------------------------------------------------------------------------------------------------------ the net
@pytest.fixture(scope="module")
def net(hip):
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=NET_H, width=NET_W, batch=len(NET_ORGS)))
    synth.load_into(n, "mid")
    return n


@pytest.fixture(scope="module")
def frames():
    return [rgb(h, w, 100 + i) for i, (h, w) in enumerate(NET_ORGS)]


@pytest.fixture(scope="module")
def oracle_input(orc, frames):
    return np.concatenate([orc.preprocess(f, NET_H, NET_W) for f in frames], 0)


def test_net_set_images_host_and_device_frames(orc, net, frames, oracle_input):
    assert {h_first(o, NET_H, NET_W) for o in NET_ORGS} == {True, False}
    assert net.blob_shape("data") == (len(frames), 3, NET_H, NET_W)
    for kind in ("host", "device"):
        net.set_blob("data", np.zeros_like(oracle_input))
        fs = frames if kind == "host" else [torch.from_numpy(f).cuda() for f in frames]
        params = net.set_images("data", fs)
        assert np.array_equal(net.get_blob("data"), oracle_input), kind
        assert [p["org_hw"] for p in params] == NET_ORGS
        assert [p["ratios"] for p in params] == [(NET_H / h, NET_W / w) for h, w in NET_ORGS]
    # a mean of its own
    m = (90.0, 100.0, 110.0)
    net.set_images("data", frames, mean_bgr=m)
    assert np.array_equal(net.get_blob("data"), np.concatenate([orc.preprocess(f, NET_H, NET_W, mean_bgr=m) for f in frames], 0))


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_set_images_forward_detect_multi_equals_the_oracle_input(net, frames, oracle_input):
    dev = [torch.from_numpy(f).cuda() for f in frames]
    params = net.set_images("data", dev)
    net.forward()
    segs, rois = net.detect_multi(params, CLASSES)
    net.set_blob("data", oracle_input)
    net.forward()
    hand = [dict(ratios=(NET_H / float(h), NET_W / float(w)), org_hw=(h, w)) for h, w in NET_ORGS]
    segs2, rois2 = net.detect_multi(hand, CLASSES)
    assert rois == rois2 and sum(rois) > 0
    total = 0
    for i in range(len(frames)):
        for c in range(len(CLASSES)):
            assert _same(segs[i][c][0], segs2[i][c][0]), (i, c)
            assert np.array_equal(segs[i][c][1], segs2[i][c][1]), (i, c)
            total += len(segs[i][c][0])
    assert total > 0


def test_set_images_refusals_leave_the_blob_unchanged(net, frames):
    net.set_images("data", frames)
    before = net.get_blob("data")
    B = len(frames)
    dev = [torch.from_numpy(f).cuda() for f in frames]
    cases = [
        (frames[:B - 1], "3 images"),                                               # count != num()
        (frames + frames[:1], "5 images"),
        (dev[:2] + frames[2:], "mixes host and device"),                            # mixed list
        (frames[:3] + [frames[3].astype(np.float32)], "frame 3 is not a uint8"),    # not uint8
        (dev[:3] + [dev[3].float()], "frame 3 is not a contiguous uint8"),
        (frames[:3] + [frames[3][:, :, :2].copy()], "frame 3 is not a uint8"),     # not [h, w, 3]
        (frames[:3] + [frames[3][:, :, 0].copy()], "frame 3 is not a uint8"),
        (frames[:3] + [np.zeros((0, 40, 3), np.uint8)], "image 3 is 0 x 40"),       # a zero dimension
        (dev[:3] + [torch.zeros((30, 0, 3), dtype=torch.uint8, device="cuda")], "image 3 is 30 x 0"),
    ]
    for fs, msg in cases:
        with pytest.raises(mnet.NetError, match=msg):
            net.set_images("data", fs)
        assert np.array_equal(net.get_blob("data"), before), msg
    with pytest.raises(mnet.NetError, match="Unknown blob name"):
        net.set_images("no_such_blob", frames)


# ---------------------------------------------------------------------------------------------------------------- the demo driver
def _read_dlm(path):
    rows = np.loadtxt(path, delimiter=",", ndmin=2) if os.path.getsize(path) else np.zeros((0, 6))
    return {int(i): rows[rows[:, 0] == i, 1:] for i in np.unique(rows[:, 0])}


def _matched(db, d1, iou_min=0.99, dscore=1e-4):
    """bench.py's fp32 batch policy: the mutual share of detections with a partner at IoU >= 0.99 and |dscore| <= 1e-4."""
    if len(db) == 0 or len(d1) == 0:
        return 1.0 if len(db) == len(d1) else 0.0
    a = np.stack([db[:, 0], db[:, 1], db[:, 0] + db[:, 2], db[:, 1] + db[:, 3]], 1)
    c = np.stack([d1[:, 0], d1[:, 1], d1[:, 0] + d1[:, 2], d1[:, 1] + d1[:, 3]], 1)
    x1 = np.maximum(a[:, None, 0], c[None, :, 0]); y1 = np.maximum(a[:, None, 1], c[None, :, 1])
    x2 = np.minimum(a[:, None, 2], c[None, :, 2]); y2 = np.minimum(a[:, None, 3], c[None, :, 3])
    inter = np.clip(x2 - x1, 0, None) * np.clip(y2 - y1, 0, None)
    iou = inter / (((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]))[:, None] + ((c[:, 2] - c[:, 0]) * (c[:, 3] - c[:, 1]))[None, :] - inter)
    near = (iou >= iou_min) & (np.abs(db[:, None, 4] - d1[None, :, 4]) <= dscore)
    return float(min(near.any(1).mean(), near.any(0).mean()))


def test_demo_driver_batch_matches_batch_one(tmp_path, capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("run_mscnn_detection", os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "tools", "run_mscnn_detection.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    deploy = tmp_path / "deploy.prototxt"
    deploy.write_text(zoo.prototxt("kitti_car/mscnn-7s-576", height=NET_H, width=NET_W))
    out = {}
    for B in (2, 1):
        d = tmp_path / f"b{B}"
        assert drv.main(["--prototxt", str(deploy), "--synthetic", "5", "--out", str(d), "--comp-id", "t", "--cls-ids", "2",
                         "--batch", str(B)]) == 0
        out[B] = _read_dlm(str(d / "t_car.txt"))
    log = capsys.readouterr().out
    assert log.count("idx 5/5, avgtime=") == 2 and log.count("detections over 5 images") == 2
    assert set(out[2]) == set(out[1]) and len(out[1]) > 0
    worst = min(_matched(out[2][i], out[1][i]) for i in out[1])
    assert worst >= 0.98, worst
