"""The render stage on the GPU: mscnn_render_detections_u8 through the HIP ABI on small synthetic packs built here (in
tests/test_gpu_track.py's style: tests/track_witness.py's pack_bytes, tests/guarded.py's arena), mscnn_net_render through the Net, and
--render-out through the drivers.  No pin on the reference (its `show` block draws through MATLAB's figure renderer): the check is
tests/render_witness.py, which tests/test_render_cpu.py holds to hand-written arrays.

The op is integer arithmetic behind four floor()s, so the bar is byte equality of every output frame, never a tolerance.

Shapes, the smallest at which the kernel can go wrong -- the boundaries of det_render.hip beside the constants they come from:
  kTileW x kTileH = 64 x 16     a workgroup's tile: frames of 37 x 53 (one tile column), 16 x 64 (exactly one tile), 70 x 130 (three
                                columns, the last 2 pixels wide; five rows, the last 6 high); boxes across x = 64 and y = 16
  kRenderThreads = 256          rows per LDS chunk: 600 boxes over one 16 x 16 region (three chunks, the order across them)
  frame bases at odd addresses  byte loads and stores only"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import guarded                                   # noqa: E402
import render_witness as rw                      # noqa: E402
import track_witness as tw                       # noqa: E402

SIZES = [(37, 53), (16, 64), (70, 130)]
VALID = [2.0, 2.0, 20.0, 10.0, 0.99]             # what the rows past a segment's count hold: a box that would show


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X: torch.cuda.is_available() is False")
    from mscnn_amd import hipapi
    hipapi.lib()
    return hipapi


def cparams(hip, p):
    return hip.render_params(p["colors"], **{k: v for k, v in p.items() if k != "colors"})


def frames_of(rng, sizes=SIZES):
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def boxes_for(rng, H, W, n_random=3):
    """Rows that straddle the tile edges and all four frame borders, a box larger than the frame, a negative origin, a box thinner than
    twice any thickness, labels forced inside their box (T < 8) and shifted left (near the right border), some random ones; scores
    around the threshold 0.3, best first as the final stage writes them."""
    rows = [[60.2, 12.4, 9.7, 8.1], [-5.3, -3.2, 20.0, 15.0], [-10.0, -10.0, W + 20.0, H + 20.0], [W - 8.0, H - 6.0, 20.0, 20.0],
            [20.0, 20.0, 4.0, 3.0], [30.0, 2.0, 12.0, 12.0], [W - 10.0, 20.0, 8.0, 8.0], [W - 1.0, 0.0, 1.0, 1.0], [0.5, H - 1.5, 3.0, 1.0]]
    for _ in range(n_random):
        x, y = rng.uniform(-8, W), rng.uniform(-8, H)
        rows.append([x, y, rng.uniform(0.6, W / 2), rng.uniform(0.6, H / 2)])
    rows = np.array(rows, np.float64)[rng.permutation(len(rows))]
    scores = np.sort(rng.uniform(0.2, 1.0, len(rows)))[::-1]
    return np.concatenate([rows, scores[:, None]], axis=1)


def ids_for(rng, n):
    return rng.choice(np.array([0, 0, 1, 2, 3, 7, 12, 40, 123456, 2147483647], np.int64), n).astype(np.int32)


def build(segs, ids, form, seg_cap=None):
    """The pack of segs[t][k] (rows or None) with VALID boxes in every row past a count, and the int32 id buffer (-1 where no row is)."""
    T, K = len(segs), len(segs[0])
    seg_cap = seg_cap or max([1] + [len(r) for fr in segs for r in fr if r is not None]) + 2
    buf, offs, cap = tw.pack_bytes(segs, seg_cap, form)
    d_at, i_at, _ = tw.pack_layout(T * K, cap)
    rows = buf[d_at:i_at].view(np.float64).reshape(cap, 5)
    used = np.zeros(cap, bool)
    idbuf = np.full(cap, 77, np.int32)           # (past a count: an id that would colour and label the VALID box)
    for t in range(T):
        for k in range(K):
            r = segs[t][k]
            if r is not None:
                o = offs[t * K + k]
                used[o:o + len(r)] = True
                if ids is not None and ids[t][k] is not None:
                    idbuf[o:o + len(r)] = ids[t][k]
    rows[~used] = VALID
    return buf, cap, idbuf


def run_op(hip, frames, segs, p, ids=None, form="merge", seg_cap=None, pass_ids=None):
    """The op on guarded buffers with every frame base at an odd address; returns the output frames after the buffer contract has been
    checked: guards intact, src / pack / ids unchanged (Arena.check), every dst byte as the witness says."""
    T, K = len(segs), len(segs[0])
    buf, cap, idbuf = build(segs, ids, form, seg_cap)
    arena = guarded.Arena("cuda")
    src = [arena.offset_view(arena.input(f, 0x5A), 1 + 2 * (b % 2)) for b, f in enumerate(frames)]
    dst = [arena.offset_view(arena.alloc(f.shape, torch.uint8), 3) for f in frames]
    assert all(t.data_ptr() % 2 == 1 for t in src + dst)
    pack = arena.input(buf, 0xA5)
    with_ids = ids is not None if pass_ids is None else pass_ids
    idt = arena.input(idbuf, -7) if with_ids else None
    hip.render_detections(cparams(hip, p), src, K, pack, cap, idt, out=dst)
    torch.cuda.synchronize()
    arena.check()
    return [d.cpu().numpy() for d in dst]


def assert_frames(got, want, what=""):
    for b, (g, w) in enumerate(zip(got, want)):
        if not np.array_equal(g, w):
            bad = np.argwhere((g != w).any(axis=2))
            raise AssertionError(f"{what} frame {b}: {len(bad)} pixels differ, first (y, x) {bad[:4].tolist()}: got {g[tuple(bad[0])]}, want {w[tuple(bad[0])]}")


def check(hip, frames, segs, p, ids=None, form="merge", what="", **kw):
    got = run_op(hip, frames, segs, p, ids, form, **kw)
    want = rw.render(frames, segs, p, ids)
    assert_frames(got, want, what)
    return got


# label, color_by, thickness, outline_alpha, fill_alpha, pixelate, with ids: every value of every knob
SETTINGS = [(1, 0, 1, 256, 0, 0, False), (2, 1, 3, 77, 77, 2, True), (3, 0, 64, 256, 256, 5, True), (0, 1, 0, 256, 77, 64, True),
            (1, 0, 3, 0, 0, 0, True), (3, 1, 1, 77, 0, 0, True)]


@pytest.mark.parametrize("form", ["merge", "image"])
@pytest.mark.parametrize("K", [1, 2])
def test_three_frames_of_their_own_sizes_are_byte_equal_to_the_witness(hip, K, form):
    rng = np.random.default_rng(100 * K + len(form))
    frames = frames_of(rng)
    segs = [[boxes_for(rng, h, w) for _ in range(K)] for h, w in SIZES]
    ids = [[ids_for(rng, len(r)) for r in fr] for fr in segs]
    drawn = 0
    for label, color_by, th, oa, fa, pix, with_ids in SETTINGS:
        p = rw.params(show_thr=0.3, thickness=th, outline_alpha=oa, fill_alpha=fa, label=label, label_scale=1 + (th == 3), color_by=color_by,
                      pixelate=pix)
        got = check(hip, frames, segs, p, ids if with_ids else None, form, what=f"{(label, color_by, th, oa, fa, pix, with_ids)}")
        drawn += sum(int((g != f).any()) for g, f in zip(got, frames))
    assert drawn == 3 * len(SETTINGS), "a frame came back unchanged: the case shows nothing"


def test_rows_that_must_be_skipped_and_segments_that_count_as_empty(hip):
    rng = np.random.default_rng(7)
    frames = frames_of(rng)
    nan, inf = float("nan"), float("inf")
    bad = np.array([[5, 5, 10, 10, nan], [nan, 5, 10, 10, 0.9], [5, inf, 10, 10, 0.9], [5, 5, -inf, 10, 0.9], [5, 5, 10, nan, 0.9],
                    [5, 5, 0, 10, 0.9], [5, 5, 10, 0, 0.9], [5, 5, -3, 10, 0.9], [5, 5, 10, -3, 0.9], [5, 5, 0.4, 10, 0.9],
                    [5, 5, 10, 10, 0.29], [5, 5, 10, 10, -inf], [5, 5, 2.0 ** 31, 10, 0.9], [-2.0 ** 30 - 1, 5, 2.0 ** 30, 10, 0.9],
                    [200, 5, 10, 10, 0.9], [5, 200, 10, 10, 0.9], [-30, 5, 10, 10, 0.9], [5, -30, 10, 10.4, 0.9], [5, 5, 10, 10, inf]], np.float64)
    p = rw.params(thickness=2, fill_alpha=77, label="both", color_by="id", pixelate=2)
    for form in ("merge", "image"):
        segs = [[bad, None], [np.zeros((0, 5)), bad], [None, np.zeros((0, 5))]]
        ids = [[np.full(len(r), 5, np.int32) if r is not None else None for r in fr] for fr in segs]
        got = run_op(hip, frames, segs, p, ids, form)
        assert_frames(got, frames, f"{form}: a row or a segment that must not be drawn was drawn;")
        assert_frames(got, rw.render(frames, segs, p, ids))
    # the same pack with one good row in front of the bad ones: it IS drawn, the rows past its count are not; and the bound itself
    good = np.concatenate([[[10, 9, 12, 6, 0.9], [-2.0 ** 30 + 8, 3, 2.0 ** 30, 4, 0.8]], bad])
    segs = [[good, None], [good[:1], good[1:2]], [None, good[:2]]]
    ids = [[np.full(len(r), 5, np.int32) if r is not None else None for r in fr] for fr in segs]
    got = check(hip, frames, segs, p, ids, "merge")
    assert all((g != f).any() for g, f in zip(got, frames))


@pytest.mark.parametrize("pixelate", [0, 2])
def test_600_boxes_over_one_region_keep_their_order_across_the_lds_chunks(hip, pixelate):
    rng = np.random.default_rng(600 + pixelate)
    frames = frames_of(rng, [(40, 70)])
    n = 600
    rows = np.stack([rng.uniform(20, 34, n), rng.uniform(12, 26, n), rng.uniform(1, 7, n), rng.uniform(1, 7, n), np.sort(rng.uniform(0.31, 1, n))[::-1]], axis=1)
    ids = [[np.arange(1, n + 1, dtype=np.int32)]]
    p = rw.params(thickness=1, label="none", color_by="id", pixelate=pixelate, colors=[tuple(int(v) for v in c) for c in rng.integers(0, 256, (31, 3))])
    got = check(hip, frames, [[rows]], p, ids)
    # the order matters in this case: painted in ascending index instead, the picture is another
    other = rw.render(frames, [[rows[::-1]]], p, [[ids[0][0][::-1]]])
    assert not np.array_equal(other[0], got[0])
    # ... and with labels, 256 and 257 rows: the chunk's edge
    for m in (256, 257):
        check(hip, frames, [[rows[:m]]], rw.params(thickness=1, label="id", color_by="id", pixelate=pixelate), [[ids[0][0][:m]]], what=f"{m} rows")


def test_label_scales_and_long_ids_and_many_slots(hip):
    rng = np.random.default_rng(33)
    frames = frames_of(rng, [(70, 130), (37, 53)])
    for scale, label, K in ((8, "score", 2), (2, "both", 3), (1, "id", 33)):      # 33: more slots than colours, k % num_colors
        segs = [[np.array([[rng.uniform(0, w - 10), rng.uniform(0, h - 10), 14, 11, 0.9 - 0.01 * k]]) for k in range(K)] for h, w in [(70, 130), (37, 53)]]
        ids = [[ids_for(rng, 1) for _ in range(K)] for _ in range(2)]
        ids[0][K - 1][:] = 2147483647            # the longest label: 10 digits, a blank, the score
        for form in ("merge", "image"):
            check(hip, frames, segs, rw.params(thickness=1, label=label, label_scale=scale, color_by="slot" if scale == 8 else "id"), ids, form,
                  what=f"scale {scale} {form}")


def raw_call(hip, p, src, dst, hs, ws, T, K, pack, cap, ids):
    arr = lambda v, ty: None if v is None else (ty * len(v))(*v)      # noqa: E731
    rc = hip.lib().mscnn_render_detections_u8(None if p is None else C.byref(p), arr(src, C.c_void_p), arr(dst, C.c_void_p), arr(hs, C.c_int),
                                              arr(ws, C.c_int), T, K, pack, cap, ids, hip._stream())
    return rc, hip.lib().mscnn_last_error().decode()


def test_every_refusal_names_its_value_and_launches_nothing(hip):
    arena = guarded.Arena("cuda")
    rng = np.random.default_rng(3)
    frames = frames_of(rng, [(8, 10), (6, 7)])
    segs = [[np.array([[1, 1, 5, 4, 0.9]])], [np.array([[1, 1, 5, 4, 0.9]])]]
    buf, cap, idbuf = build(segs, None, "merge")
    src = [arena.input(f, 0x5A) for f in frames]
    dst = [arena.alloc(f.shape, torch.uint8) for f in frames]
    big = arena.alloc((2 * 8 * 10 * 3,), torch.uint8)
    pack, ids = arena.input(np.concatenate([buf, np.zeros(16, np.uint8)]), 0xA5), arena.input(np.concatenate([idbuf, idbuf]), -7)
    S, D, PK, ID = [t.data_ptr() for t in src], [t.data_ptr() for t in dst], pack.data_ptr(), ids.data_ptr()
    hs, ws = [8, 6], [10, 7]
    ok = dict(show_thr=0.3, thickness=2, outline_alpha=256, fill_alpha=0, label=1, label_scale=1, color_by=0, pixelate=0)

    def P(**kw):
        colors = kw.pop("colors", rw.PALETTE)
        n = kw.pop("num_colors", None)
        p = hip.render_params(colors, **dict(ok, **kw))
        if n is not None:
            p.num_colors = n
        return p

    base = dict(p=P(), src=S, dst=D, hs=hs, ws=ws, T=2, K=1, pack=PK, cap=cap, ids=None)
    cases = [
        (dict(p=None), "render_detections: null pointer"), (dict(src=None), "render_detections: null pointer"),
        (dict(dst=None), "render_detections: null pointer"), (dict(hs=None), "render_detections: null pointer"),
        (dict(ws=None), "render_detections: null pointer"), (dict(pack=None), "render_detections: null pointer"),
        (dict(src=[S[0], None]), "render_detections: source frame 1 is a null pointer"),
        (dict(dst=[None, D[1]]), "render_detections: destination frame 0 is a null pointer"),
        (dict(T=0), "render_detections: num_frames 0"), (dict(K=0), "render_detections: num_slots 0"), (dict(cap=0), "render_detections: cap 0"),
        (dict(K=1 << 15, cap=1 << 15), "render_detections: 2 frames x 32768 slots x 32768 pack rows is past 2^31 - 1"),
        (dict(hs=[8, 0]), "render_detections: frame 1 has bad shape 0 x 7"), (dict(ws=[-1, 7]), "render_detections: frame 0 has bad shape 8 x -1"),
        (dict(p=P(thickness=-1)), "thickness -1 is outside [0, 64]"), (dict(p=P(thickness=65)), "thickness 65 is outside [0, 64]"),
        (dict(p=P(outline_alpha=257)), "outline_alpha 257 is outside [0, 256]"), (dict(p=P(fill_alpha=-1)), "fill_alpha -1 is outside [0, 256]"),
        (dict(p=P(label=4)), "label 4 is outside [0, 3]"), (dict(p=P(label=-1)), "label -1 is outside [0, 3]"),
        (dict(p=P(label_scale=0)), "label_scale 0 is outside [1, 8]"), (dict(p=P(label_scale=9)), "label_scale 9 is outside [1, 8]"),
        (dict(p=P(color_by=2), ids=ID), "color_by 2 is neither 0 (slot) nor 1 (track id)"),
        (dict(p=P(pixelate=1)), "pixelate 1 is neither 0 nor inside [2, 64]"), (dict(p=P(pixelate=65)), "pixelate 65 is neither 0 nor inside [2, 64]"),
        (dict(p=P(pixelate=-2)), "pixelate -2 is neither 0 nor inside [2, 64]"),
        (dict(p=P(num_colors=0)), "num_colors 0 is outside [1, 32]"), (dict(p=P(num_colors=33)), "num_colors 33 is outside [1, 32]"),
        (dict(p=P(show_thr=float("nan"))), "show_thr is NaN"),
        (dict(p=P(label=2)), "label 2, color_by 0 need the track ids, track_ids_dev is null"),
        (dict(p=P(label=3)), "label 3, color_by 0 need the track ids, track_ids_dev is null"),
        (dict(p=P(color_by=1)), "label 1, color_by 1 need the track ids, track_ids_dev is null"),
        (dict(pack=PK + 8), "pack_dev must be 16-byte aligned"), (dict(ids=ID + 2), "track_ids_dev must be 4-byte aligned"),
        (dict(dst=[S[0], D[1]]), "render_detections: destination frame 0 overlaps source frame 0"),
        (dict(dst=[D[0], S[0] + 30]), "render_detections: destination frame 1 overlaps source frame 0"),
        (dict(dst=[S[1] - 10, D[1]]), "render_detections: destination frame 0 overlaps source frame 1"),
        (dict(dst=[big.data_ptr(), big.data_ptr() + 8 * 10 * 3 - 1]), "render_detections: destination frame 0 overlaps destination frame 1"),
    ]
    for change, text in cases:
        rc, err = raw_call(hip, **dict(base, **change))
        assert rc != 0 and text in err, (change, rc, err)
    torch.cuda.synchronize()
    arena.check()
    assert all(guarded.all_poison(d) for d in dst) and guarded.all_poison(big), "a refused call wrote a frame"
    # the wrapper names a bad name itself, and the call that is not refused draws
    with pytest.raises(hip.MscnnError, match="label 'scores' is none of"):
        hip.render_params(rw.PALETTE, label="scores")
    rc, err = raw_call(hip, **dict(base, dst=[big.data_ptr(), big.data_ptr() + 8 * 10 * 3], ids=ID, p=P(label=3, color_by=1)))
    assert rc == 0, err
    torch.cuda.synchronize()
    want = rw.render(frames, segs, rw.params(label=3, color_by=1), [[idbuf[0:1]], [idbuf[cap // 2:cap // 2 + 1]]])
    got = big.cpu().numpy()
    assert np.array_equal(got[:240].reshape(8, 10, 3), want[0]) and np.array_equal(got[240:240 + 126].reshape(6, 7, 3), want[1])


def test_a_chunk_of_more_than_32_frames_takes_a_second_launch(hip):
    rng = np.random.default_rng(34)
    sizes = [(5 + (b % 7), 9 + (b % 5)) for b in range(35)]
    frames = frames_of(rng, sizes)
    segs = [[np.array([[b % 4, b % 3, 4 + b % 3, 3 + b % 2, 0.9]])] for b in range(35)]
    check(hip, frames, segs, rw.params(thickness=1, label="none", fill_alpha=77, colors=[(9, 200, 30)]))


# ---- the Net -------------------------------------------------------------------------------------------------------------------------------------
import test_gpu_seq as gq                        # noqa: E402  (clip_net, small_u8: the small synthetic frames of the Net tracker tests)
import test_gpu_track as gt                      # noqa: E402  (thresholds, gap_thr, driver, run_main, common_of)

from mscnn_amd import net as mnet                # noqa: E402


def segs_of(res):
    return [[seg[0] for seg in img] for img in res[0]]


def test_net_render_is_the_witness_on_the_returned_detections_and_ids_and_steps_nothing(hip):
    T, classes = 2, [2, 3]
    imgs = [gq.small_u8(47, 2 * t) for t in range(T)]
    n, params, R = gq.clip_net(imgs)
    with pytest.raises(mnet.NetError, match="render: no pack to render"):
        n.render(imgs)
    plain = n.detect_multi(params, classes)
    hi, lo = gt.thresholds(plain)
    scores = np.concatenate([seg[0][:, 4] for img in plain[0] for seg in img])
    thr = gt.gap_thr(scores, 0.8)
    # without a tracker: scores and slot colours; ids are refused, naming the reason
    got = n.render(imgs, thr=thr, label="score", pixelate=0)
    want = rw.render(imgs, segs_of(plain), rw.params(show_thr=thr, label="score"))
    assert_frames(got, want, "no tracker:")
    assert all((g != f).any() for g, f in zip(got, imgs)), "nothing was drawn: the case shows nothing"
    for kw in (dict(label="id"), dict(label="both"), dict(color_by="id")):
        with pytest.raises(mnet.NetError, match=r"render: label \d, color_by \d need track ids, and that call ran no tracker"):
            n.render(imgs, thr=thr, **kw)
    with pytest.raises(mnet.NetError, match="render: 1 frames, that call had 2 images"):
        n.render(imgs[:1])
    with pytest.raises(mnet.NetError, match=r"render_detections: thickness 65 is outside \[0, 64\]"):
        n.render(imgs, thickness=65)
    with pytest.raises(mnet.NetError, match="label 'scores' is none of"):
        n.render(imgs, label="scores")
    # with the tracker: ids in the labels and the colours; host and device frames give equal bytes; nothing is stepped
    n.set_tracker(high_thr=hi, low_thr=lo, match_thr=0.2, max_tracks=64)
    res = n.detect_multi(params, classes)
    ids, state = n.detect_tracks(), n.tracker_state(raw=True)
    assert any((i > 0).any() for fr in ids for i in fr)
    kw = dict(thr=thr, thickness=3, label="both", color_by="id", pixelate=4, outline_alpha=200, fill_alpha=40, label_scale=2)
    got = n.render(imgs, **kw)
    p = rw.params(show_thr=thr, thickness=3, label="both", color_by="id", pixelate=4, outline_alpha=200, fill_alpha=40, label_scale=2)
    assert_frames(got, rw.render(imgs, segs_of(res), p, ids), "tracked:")
    dev = [torch.from_numpy(f).cuda() for f in imgs]
    before = [d.clone() for d in dev]
    on_dev = n.render(dev, **kw)
    torch.cuda.synchronize()
    assert all(o.is_cuda for o in on_dev) and all(torch.equal(a, b) for a, b in zip(dev, before))
    assert_frames([o.cpu().numpy() for o in on_dev], got, "device frames:")
    assert gt.same_ids(n.detect_tracks(), ids) and np.array_equal(n.tracker_state(raw=True), state), "render stepped the tracks"
    again = n.detect_multi(params, classes)
    assert gt.flat_multi(again) == gt.flat_multi(res)
    # the merge's pack (own row offsets), ids behind it
    n.detect_merge_begin(T, len(classes), R)
    n.detect_merge_add(params, classes)
    merged = n.detect_merge_end()
    mids = n.detect_tracks()
    assert_frames(n.render(imgs, **kw), rw.render(imgs, segs_of(merged), p, mids), "merge:")
    # another call has used the Net's pack block since: refused
    n.set_tracker(None)
    n.detect_image(0, 2, params[0]["ratios"], params[0]["org_hw"])
    with pytest.raises(mnet.NetError, match="render: no pack to render"):
        n.render(imgs)


# ---- the drivers ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tool,common", [("run_mscnn_detection.py", ["--cls-ids", "2"]), ("run_cascademscnn.py", gq.CASCADE[:-2])])
def test_driver_render_out_writes_the_witness_pngs_and_leaves_the_result_files_alone(hip, tmp_path, monkeypatch, capsys, tool, common):
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
    thr = gt.gap_thr(np.concatenate([r[:, 4] for fr in segs for r in fr]), 0.7)
    out = tmp_path / "png"
    drawn = gt.run_main(drv, tmp_path / "drawn", *common, "--render-out", str(out), "--show-thr", repr(thr), "--pixelate", "3")
    capsys.readouterr()
    assert drawn == plain, "--render-out changed a result file"
    assert sorted(os.listdir(out)) == ["000007.png", "000008.png"]
    want = rw.render(imgs, segs, rw.params(show_thr=thr, label="score", pixelate=3))
    got = [np.asarray(Image.open(out / f"{7 + t:06d}.png").convert("RGB")) for t in range(2)]
    assert_frames(got, want)
    assert all((g != f).any() for g, f in zip(got, imgs)), "nothing was drawn: the case shows nothing"


def test_driver_render_flag_refusals(hip, monkeypatch, capsys):
    drv = gt.driver("run_mscnn_detection.py", monkeypatch)
    base = ["--model", "kitti_car/mscnn-7s-576", "--synthetic", "1"]
    for extra, text in ((["--show-thr", "0.5"], "belong to --render-out"), (["--pixelate", "4"], "belong to --render-out"),
                        (["--render-out", "x", "--render-label", "id"], "it needs --track"), (["--render-out", "x", "--render-color", "id"], "it needs --track"),
                        (["--render-out", "x", "--pixelate", "1"], "--pixelate 1: the mosaic's block edge, 2 .. 64"),
                        (["--render-out", "x", "--proposals-only", "--proposals-out", "p"], "--render-out draws the detections")):
        with pytest.raises(SystemExit):
            drv.parse_args(base + extra)
        assert text in capsys.readouterr().err, extra
    a = drv.parse_args(base + ["--render-out", "x", "--track", "--render-label", "both", "--render-color", "id", "--batch", "3", "--streams", "3"])
    assert drv.show_thr_of(a) == 0.3 and a.render_label == "both"
    assert drv.show_thr_of(drv.parse_args(["--model", "caltech/mscnn-8s-720", "--synthetic", "1", "--render-out", "x"])) == 0.1
