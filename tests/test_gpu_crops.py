"""The crop stage on the GPU: mscnn_net_crops through Net.crops on the small synthetic clip net of the tracker / render tests, and
--crops-out through the drivers.  No pin on the reference (its scripts cut no patches).  Two checks, both for equality, never a
tolerance: the windows and their order against tests/crops_witness.py (which tests/test_crops_cpu.py holds to hand-written windows and
to mscnn_net_crop_window), and every patch against the single-frame op (hipapi.preprocess) on a host copy of its window -- the
definition of a view's slice, bit for bit.

Shapes: frames of 120 x 400 into a 2 x 96 x 320 forward; patches of 24 x 12 unless a case needs another size (4 x 4 under windows of at
least 5 x 5: every window shrinks; 96 x 96 over frames of 80 x 90: every window grows; more than 32 crops: the views op's table
chunk)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import crops_witness as cw                       # noqa: E402
import test_gpu_seq as gq                        # noqa: E402  (clip_net, small_u8, CASCADE)
import test_gpu_track as gt                      # noqa: E402  (thresholds, gap_thr, driver, run_main, common_of, flat_multi, same_ids)

from mscnn_amd import net as mnet                # noqa: E402
from mscnn_amd import zoo                        # noqa: E402

CLASSES = [2, 3]
SIZE = (24, 12)
MEAN = (104.0, 117.0, 123.0)
POISON = -7777.25
ALL = -1e300                                     # a threshold under every finite score


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X: torch.cuda.is_available() is False")
    from mscnn_amd import hipapi
    hipapi.lib()
    return hipapi


@pytest.fixture(autouse=True)
def stop_at_a_device_error():
    """A device error ends the session: no later test starts work on a device that has reported one."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported an error: {e}", returncode=3)


class Scene:
    """Two frames forwarded as one batch, once; every test starts from detect() -- the same forward, a fresh pack."""

    def __init__(self):
        self.imgs = [gq.small_u8(47, 2 * t) for t in range(2)]
        self.net, self.params, self.R = gq.clip_net(self.imgs)
        try:
            self.net.crops(self.imgs, size=SIZE)
            self.no_pack = ""
        except mnet.NetError as e:
            self.no_pack = str(e)
        self.plain = self.net.detect_multi(self.params, CLASSES)
        self.scores = np.concatenate([seg[0][:, 4] for img in self.plain[0] for seg in img])
        self.thr = gt.gap_thr(self.scores, 0.5)

    def detect(self):
        res = self.net.detect_multi(self.params, CLASSES)
        assert gt.flat_multi(res) == gt.flat_multi(self.plain)
        return res

    def reforward(self):
        self.net.set_images("data", self.imgs)
        self.net.forward()


@pytest.fixture(scope="module")
def scene(hip):
    return Scene()


def segs_of(res):
    return [[seg[0] for seg in img] for img in res[0]]


def as_tuples(info):
    return [tuple(int(v) for v in rec) for rec in info]


def witness(frames, segs, ids=None, **kw):
    """(info tuples, dropped) of crops_witness for Net.crops' keywords; max_crops None = no bound."""
    kw = dict(kw)
    if kw.get("max_crops") is None:
        kw["max_crops"] = 1 << 30
    return cw.crops(frames, segs, cw.params(**kw), ids)


def host(patches):
    return patches if isinstance(patches, np.ndarray) else patches.cpu().numpy()


def assert_patches(hip, frames, patches, info, size, mean=(0.0, 0.0, 0.0), which=None):
    """Every patch (or those of `which`) is the single-frame op on a contiguous host copy of its window, bit for bit."""
    patches = host(patches)
    assert patches.shape == (len(info), 3, size[0], size[1]) and patches.dtype == np.float32
    for i in (range(len(info)) if which is None else which):
        r = info[i]
        win = np.ascontiguousarray(frames[int(r["frame"])][int(r["y0"]):int(r["y0"]) + int(r["h"]), int(r["x0"]):int(r["x0"]) + int(r["w"])])
        assert win.shape == (int(r["h"]), int(r["w"]), 3), (i, r)
        want = hip.preprocess(torch.from_numpy(win).cuda(), size[0], size[1], mean)[0].cpu().numpy()
        assert np.array_equal(patches[i].view(np.uint32), want.view(np.uint32)), f"patch {i} {r}: max |diff| {np.abs(patches[i] - want).max()}"


def same_bits(a, b):
    a, b = host(a), host(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_without_a_pack_the_call_is_refused(scene):
    assert "crops: no pack" in scene.no_pack, scene.no_pack


def test_after_detect_multi_info_is_the_witness_and_every_patch_the_single_frame_op(hip, scene):
    res = scene.detect()
    kw = dict(size=SIZE, thr=scene.thr, mean=MEAN)
    patches, info = scene.net.crops(scene.imgs, **kw)
    want, dropped = witness(scene.imgs, segs_of(res), **kw)
    print(f"{len(info)} crops of {len(scene.scores)} rows, thr {scene.thr:.6f}")
    assert as_tuples(info) == want and info.dropped == dropped == 0
    assert len(info) >= 2, "fewer than 2 crops: the case shows nothing"
    assert int((scene.scores < scene.thr).sum()) >= 1 and len(info) < len(scene.scores), "no row was skipped by thr: the case shows nothing"
    assert isinstance(patches, np.ndarray)
    assert_patches(hip, scene.imgs, patches, info, SIZE, MEAN)
    # one slot only
    one, info1 = scene.net.crops(scene.imgs, slot=1, **kw)
    assert as_tuples(info1) == [w for w in want if w[1] == 1] and same_bits(one, patches[[i for i, w in enumerate(want) if w[1] == 1]])


def test_every_window_larger_than_the_patch_and_every_window_smaller(hip, scene):
    res = scene.detect()
    kw = dict(size=(4, 4), thr=ALL, min_size=5)
    patches, info = scene.net.crops(scene.imgs, **kw)
    assert as_tuples(info) == witness(scene.imgs, segs_of(res), **kw)[0]
    assert len(info) >= 2 and int(info["w"].min()) >= 5 and int(info["h"].min()) >= 5, "no window to shrink: the case shows nothing"
    assert_patches(hip, scene.imgs, patches, info, (4, 4))
    small = [np.ascontiguousarray(f[:80, :90]) for f in scene.imgs]             # smaller than 96 in both directions
    try:
        params = scene.net.set_images("data", small)
        scene.net.forward()
        res = scene.net.detect_multi(params, CLASSES)
        kw = dict(size=(96, 96), thr=ALL)
        patches, info = scene.net.crops(small, **kw)
        assert as_tuples(info) == witness(small, segs_of(res), **kw)[0]
        assert len(info) >= 2 and int(info["w"].max()) <= 90 and int(info["h"].max()) <= 80, "no window to enlarge: the case shows nothing"
        assert_patches(hip, small, patches, info, (96, 96))
    finally:
        scene.reforward()


def test_fit_and_shift_with_context(hip, scene):
    res = scene.detect()
    kw = dict(size=SIZE, thr=scene.thr, context=1.5, fit=True, border="shift", mean=MEAN)
    patches, info = scene.net.crops(scene.imgs, **kw)
    want, _ = witness(scene.imgs, segs_of(res), **kw)
    assert as_tuples(info) == want and len(info) >= 2
    plain, _ = witness(scene.imgs, segs_of(res), size=SIZE, thr=scene.thr)
    assert [w[4:] for w in want] != [w[4:] for w in plain], "the knobs changed no window: the case shows nothing"
    assert_patches(hip, scene.imgs, patches, info, SIZE, MEAN)


def test_host_frames_and_device_frames_give_the_same_bits_and_the_frames_stay_untouched(hip, scene):
    scene.detect()
    kw = dict(size=SIZE, thr=scene.thr, context=1.5, mean=MEAN)
    hp, hi = scene.net.crops(scene.imgs, **kw)
    dev = [torch.from_numpy(f).cuda() for f in scene.imgs]
    before = [d.clone() for d in dev]
    dp, di = scene.net.crops(dev, **kw)
    torch.cuda.synchronize()
    assert dp.is_cuda and len(hi) >= 2 and as_tuples(di) == as_tuples(hi) and same_bits(dp, hp)
    assert all(torch.equal(a, b) for a, b in zip(dev, before))


def test_device_out_and_host_out_give_the_same_bits_and_leave_the_slices_behind_them_alone(hip, scene):
    scene.detect()
    kw = dict(size=SIZE, thr=scene.thr, mean=MEAN)
    ref, info = scene.net.crops(scene.imgs, **kw)
    n = len(info)
    assert n >= 2
    dev = [torch.from_numpy(f).cuda() for f in scene.imgs]
    for frames in (scene.imgs, dev):
        hout = np.full((n + 3, 3) + SIZE, POISON, np.float32)
        dout = torch.full((n + 3, 3) + SIZE, POISON, dtype=torch.float32, device="cuda")
        hp, hi = scene.net.crops(frames, out=hout, **kw)
        dp, di = scene.net.crops(frames, out=dout, **kw)
        torch.cuda.synchronize()
        assert as_tuples(hi) == as_tuples(di) == as_tuples(info) and hi.dropped == di.dropped == 0
        assert same_bits(hp, ref) and same_bits(dp, ref) and same_bits(hout[:n], ref) and same_bits(dout[:n], ref)
        assert (hout[n:] == POISON).all() and bool((dout[n:] == POISON).all()), "a slice past num_crops was written"


def test_max_crops_one_short_drops_exactly_one_and_keeps_the_first(hip, scene):
    scene.detect()
    kw = dict(size=SIZE, thr=scene.thr)
    ref, info = scene.net.crops(scene.imgs, **kw)
    n = len(info)
    assert n >= 2
    got, ginfo = scene.net.crops(scene.imgs, max_crops=n - 1, **kw)
    assert ginfo.dropped == 1 and as_tuples(ginfo) == as_tuples(info)[:n - 1] and same_bits(got, ref[:n - 1])
    got, ginfo = scene.net.crops(scene.imgs, max_crops=1, **kw)
    assert ginfo.dropped == n - 1 and as_tuples(ginfo) == as_tuples(info)[:1] and same_bits(got, ref[:1])


def test_more_than_32_crops_cross_the_table_chunk_of_the_views_op(hip):
    imgs = [gq.small_u8(47, 2 * t) for t in range(8)]
    classes = [2, 3, 4, 5]
    n, params, _ = gq.clip_net(imgs)
    res = n.detect_multi(params, classes)
    kw = dict(size=SIZE, thr=ALL, mean=MEAN)
    want, _ = witness(imgs, segs_of(res), **kw)
    print(f"{len(want)} crops over 8 frames")
    assert len(want) >= 34, f"the witness counts {len(want)} crops: the table chunk of 32 is not crossed with crops 31 .. 33 behind it"
    patches, info = n.crops(imgs, **kw)
    assert as_tuples(info) == want and info.dropped == 0
    assert len({int(f) for f in info["frame"]}) >= 2
    assert_patches(hip, imgs, patches, info, SIZE, MEAN, which=(0, 31, 32, 33, len(want) - 1))
    # the same from device frames into a device buffer
    dp, di = n.crops([torch.from_numpy(f).cuda() for f in imgs], **kw)
    torch.cuda.synchronize()
    assert as_tuples(di) == want and same_bits(dp, patches)


def test_with_the_tracker_on_the_ids_come_along_and_nothing_is_stepped(hip, scene):
    n = scene.net
    hi, lo = gt.thresholds(scene.plain)
    try:
        n.set_tracker(high_thr=hi, low_thr=lo, match_thr=0.2, max_tracks=64)
        res = n.detect_multi(scene.params, CLASSES)
        ids, state = n.detect_tracks(), n.tracker_state(raw=True)
        flat = np.concatenate([i for fr in ids for i in fr])
        assert (flat > 0).any() and (flat <= 0).any(), "every row tracked, or none: the case shows nothing"
        kw = dict(size=SIZE, thr=ALL, mean=MEAN)
        patches, info = n.crops(scene.imgs, **kw)
        want, _ = witness(scene.imgs, segs_of(res), ids, **kw)
        assert as_tuples(info) == want
        for r in info:
            assert int(r["track_id"]) == int(ids[int(r["frame"])][int(r["slot"])][int(r["row"])])
        tp, tinfo = n.crops(scene.imgs, tracked_only=True, **kw)
        keep = [i for i, w in enumerate(want) if w[3] > 0]
        assert 0 < len(keep) < len(want) and as_tuples(tinfo) == [want[i] for i in keep] and same_bits(tp, patches[keep])
        assert as_tuples(tinfo) == witness(scene.imgs, segs_of(res), ids, tracked_only=True, **kw)[0]
        assert_patches(hip, scene.imgs, tp, tinfo, SIZE, MEAN, which=range(min(3, len(tinfo))))
        assert gt.same_ids(n.detect_tracks(), ids) and np.array_equal(n.tracker_state(raw=True), state), "crops stepped the tracks"
        again = n.detect_multi(scene.params, CLASSES)
        assert gt.flat_multi(again) == gt.flat_multi(res) == gt.flat_multi(scene.plain)
    finally:
        n.set_tracker(None)


def test_after_detect_merge_end_the_merged_lists_and_after_detect_image_refused_again(hip, scene):
    n = scene.net
    n.detect_merge_begin(2, len(CLASSES), scene.R)
    n.detect_merge_add(scene.params, CLASSES)
    merged = n.detect_merge_end()
    kw = dict(size=SIZE, thr=scene.thr, mean=MEAN)
    patches, info = n.crops(scene.imgs, **kw)
    want, _ = witness(scene.imgs, segs_of(merged), **kw)
    assert as_tuples(info) == want and len(want) >= 2 and len({w[1] for w in want}) == 2, "one slot only: own row offsets are not shown"
    assert_patches(hip, scene.imgs, patches, info, SIZE, MEAN)
    n.detect_image(0, 2, scene.params[0]["ratios"], scene.params[0]["org_hw"])
    with pytest.raises(mnet.NetError, match="crops: no pack"):
        n.crops(scene.imgs, **kw)


def test_render_then_crops_is_crops_then_render(hip, scene):
    n = scene.net
    kw = dict(size=SIZE, thr=scene.thr, context=1.5)
    scene.detect()
    r1 = n.render(scene.imgs, thr=scene.thr)
    c1, i1 = n.crops(scene.imgs, **kw)
    scene.detect()
    c2, i2 = n.crops(scene.imgs, **kw)
    r2 = n.render(scene.imgs, thr=scene.thr)
    assert len(i1) >= 2 and as_tuples(i1) == as_tuples(i2) and same_bits(c1, c2)
    assert all(np.array_equal(a, b) for a, b in zip(r1, r2)) and any((a != f).any() for a, f in zip(r1, scene.imgs))


def test_on_a_callers_stream_the_results_are_those_of_the_default_stream(hip, scene):
    n = scene.net
    scene.detect()
    kw = dict(size=SIZE, thr=scene.thr, mean=MEAN)
    ref, rinfo = n.crops(scene.imgs, **kw)
    dev = [torch.from_numpy(f).cuda() for f in scene.imgs]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), mnet.on_stream(side):
        hp, hinfo = n.crops(scene.imgs, **kw)                                 # host out: back behind one synchronisation of that stream
        dout = torch.full((len(rinfo) + 1, 3) + SIZE, POISON, dtype=torch.float32, device="cuda")
        dp, dinfo = n.crops(dev, out=dout, **kw)                              # device out: asynchronous on that stream
        side.synchronize()
    torch.cuda.synchronize()
    assert len(rinfo) >= 2 and as_tuples(hinfo) == as_tuples(dinfo) == as_tuples(rinfo)
    assert same_bits(hp, ref) and same_bits(dp, ref) and bool((dout[len(rinfo):] == POISON).all())


def test_every_refusal_names_its_value_and_leaves_out_poisoned(hip, scene):
    n = scene.net
    scene.detect()
    K = len(CLASSES)
    hout = np.full((4, 3) + SIZE, POISON, np.float32)
    dout = torch.full((4, 3) + SIZE, POISON, dtype=torch.float32, device="cuda")
    dev = [torch.from_numpy(f).cuda() for f in scene.imgs]
    nan, inf = float("nan"), float("inf")
    cases = [(dict(thr=nan), "crops: thr is NaN"), (dict(context=0.5), "crops: context 0.5 is outside [1, 16]"),
             (dict(context=17.0), "crops: context 17 is outside [1, 16]"), (dict(context=nan), "crops: context nan is outside [1, 16]"),
             (dict(fit=2), "crops: fit 2 is neither 0 nor 1"), (dict(border=2), "crops: border 2 is neither 0 (clip) nor 1 (shift)"),
             (dict(border=-1), "crops: border -1 is neither"), (dict(min_size=0), "crops: min_size 0 is below 1"),
             (dict(max_crops=0), "crops: max_crops 0 is below 1"), (dict(max_crops=-3), "crops: max_crops -3 is below 1"),
             (dict(slot=K), f"crops: slot {K} is outside [-1, {K})"), (dict(slot=-2), "crops: slot -2 is below -1"),
             (dict(tracked_only=2), "crops: tracked_only 2 is neither 0 nor 1"),
             (dict(tracked_only=True), "crops: tracked_only 1 needs track ids, and that call ran no tracker"),
             (dict(mean=(0, inf, 0)), "crops: mean_bgr[1] inf is not finite"), (dict(mean=(nan, 0, 0)), "crops: mean_bgr[0] nan is not finite")]
    for kw, text in cases:
        for frames, out in ((scene.imgs, hout), (dev, dout)):
            with pytest.raises(mnet.NetError) as e:
                n.crops(frames, out=out, **dict(dict(size=SIZE, thr=scene.thr), **kw))
            assert text in str(e.value), (kw, str(e.value))
    for size, text in (((0, 12), "crops: out_h 0 is outside [1, 1024]"), ((1025, 12), "crops: out_h 1025 is outside"),
                       ((24, 0), "crops: out_w 0 is outside [1, 1024]"), ((24, 1025), "crops: out_w 1025 is outside")):
        with pytest.raises(mnet.NetError) as e:
            n.crops(scene.imgs, size=size, thr=scene.thr)
        assert text in str(e.value), (size, str(e.value))
    with pytest.raises(mnet.NetError, match="crops: 1 frames, that call had 2 images"):
        n.crops(scene.imgs[:1], out=hout, size=SIZE)
    with pytest.raises(mnet.NetError, match="crops: 3 frames, that call had 2 images"):
        n.crops(dev + dev[:1], out=dout, size=SIZE)
    with pytest.raises(mnet.NetError, match="crops: a list that mixes host and device frames"):
        n.crops([scene.imgs[0], dev[1]], out=hout, size=SIZE)
    # the C entry itself: null pointers, a null frame, frame sizes
    L = mnet.lib()
    p = mnet.crops_params(size=SIZE, thr=scene.thr, max_crops=4)
    info = np.zeros(4, mnet.CROP_INFO)
    nc, nd = C.c_int(-5), C.c_int(-5)
    ptrs = [d.data_ptr() for d in dev]

    def raw(**kw):
        a = dict(frames=ptrs, hs=[120, 120], ws=[400, 400], count=2, p=C.byref(p), out=dout.data_ptr(), info=info.ctypes.data, nc=C.byref(nc),
                 nd=C.byref(nd))
        a.update(kw)
        arr = lambda v, ty: None if v is None else (ty * len(v))(*v)      # noqa: E731
        rc = L.mscnn_net_crops(n._h, arr(a["frames"], C.c_void_p), 1, arr(a["hs"], C.c_int), arr(a["ws"], C.c_int), a["count"], a["p"], a["out"], 1,
                               a["info"], a["nc"], a["nd"])
        return rc, L.mscnn_net_last_error().decode()

    for kw, text in ((dict(frames=None), "crops: null pointer"), (dict(hs=None), "crops: null pointer"), (dict(ws=None), "crops: null pointer"),
                     (dict(p=None), "crops: null pointer"), (dict(out=None), "crops: null pointer"), (dict(info=None), "crops: null pointer"),
                     (dict(nc=None), "crops: null pointer"), (dict(nd=None), "crops: null pointer"),
                     (dict(frames=[ptrs[0], None]), "crops: frame 1 is 120 x 400 at a null pointer"),
                     (dict(hs=[0, 120]), "crops: frame 0 is 0 x 400"), (dict(ws=[400, -1]), "crops: frame 1 is 120 x -1"),
                     (dict(hs=[120, (1 << 30) + 1]), "crops: frame 1 is 1073741825 x 400")):
        rc, err = raw(**kw)
        assert rc != 0 and text in err, (kw, rc, err)
    assert nc.value == -5 and nd.value == -5
    graph = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=96, width=320, max_nms_num=200), device=-1)
    with pytest.raises(mnet.NetError, match=r"crops: the net was built with device -1 \(graph only\)"):
        graph.crops(scene.imgs, out=hout, size=SIZE)
    torch.cuda.synchronize()
    assert (hout == POISON).all() and bool((dout == POISON).all()), "a refused call wrote a patch"
    # and the call that is not refused writes
    rc, err = raw()
    torch.cuda.synchronize()
    assert rc == 0 and nc.value >= 1 and not bool((dout[:nc.value] == POISON).any()), err


# ---- the drivers ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tool,common", [("run_mscnn_detection.py", ["--cls-ids", "2"]), ("run_cascademscnn.py", gq.CASCADE[:-2])])
def test_driver_crops_out_writes_the_witness_windows_as_pngs_and_leaves_the_result_files_alone(hip, tmp_path, monkeypatch, capsys, tool, common):
    from PIL import Image
    drv = gt.driver(tool, monkeypatch)
    images = tmp_path / "images"
    os.makedirs(images)
    imgs = [gq.small_u8(47, 2 * t) for t in range(2)]
    for t, f in enumerate(imgs):
        Image.fromarray(f, "RGB").save(images / f"{7 + t:06d}.png")
    common = gt.common_of(tool, [c for c in common], tmp_path) + ["--images", str(images), "--batch", "2"]
    seen = []
    name = "detect_multi" if tool == "run_mscnn_detection.py" else "detect_cascade_multi"
    real = getattr(mnet.Net, name)

    def spy(self, *a, **k):
        out = real(self, *a, **k)
        seen.append(out)
        return out

    monkeypatch.setattr(mnet.Net, name, spy)
    plain = gt.run_main(drv, tmp_path / "plain", *common)
    per_image = seen[0][0]
    if tool == "run_cascademscnn.py":            # [image][output][class] -> [image][slot]
        per_image = [[seg for out in img for seg in out] for img in per_image]
    segs = [[seg[0] for seg in img] for img in per_image]
    thr = gt.gap_thr(np.concatenate([r[:, 4] for fr in segs for r in fr]), 0.5)
    out = tmp_path / "crops"
    cut = gt.run_main(drv, tmp_path / "cut", *common, "--crops-out", str(out), "--crop-size", "20x10", "--crop-thr", repr(thr), "--crop-context", "1.5",
                      "--crop-fit", "--crop-border", "shift")
    capsys.readouterr()
    assert cut == plain, "--crops-out changed a result file"
    want, _ = witness(imgs, segs, size=(20, 10), thr=thr, context=1.5, fit=True, border="shift")
    assert len(want) >= 2, "fewer than 2 crops: the case shows nothing"
    assert sorted(os.listdir(out)) == sorted(f"{7 + b:06d}_{k}_{j}.png" for b, k, j, *_ in want)
    for b, k, j, _, x0, y0, w, h in want:
        win = np.ascontiguousarray(imgs[b][y0:y0 + h, x0:x0 + w])
        v = hip.preprocess(torch.from_numpy(win).cuda(), 20, 10, (0.0, 0.0, 0.0))[0].cpu().numpy().astype(np.float64)
        rgb = np.minimum(np.maximum(np.floor(v + .5), 0), 255).astype(np.uint8)[::-1].transpose(1, 2, 0)
        got = np.asarray(Image.open(out / f"{7 + b:06d}_{k}_{j}.png").convert("RGB"))
        assert np.array_equal(got, rgb), (b, k, j)
