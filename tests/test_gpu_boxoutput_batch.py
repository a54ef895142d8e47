"""BoxOutput for every image of a batch side by side (mscnn_boxoutput_batch_fwd_f32) on the GPU: every output word -- rois, props,
anchor ids, both count words, and everything the op does NOT write up to a guard band behind the buffers -- equals the per-image
op's on the same heads, and the rows equal the oracle's.  Integer / compare work: np.array_equal everywhere, no tolerance.  Net
level: a batched forward with the switch on and off gives the same blobs and the same detections."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from mscnn_amd import net as mnet, synth, zoo   # noqa: E402

KITTI_HEADS = dict(shapes=[(18, 60), (18, 60), (9, 30), (9, 30), (5, 15), (5, 15), (3, 8)],      # as tests/test_gpu_ops.py
                   field=[60, 84, 120, 168, 240, 336, 480], ds=[8, 8, 16, 16, 32, 32, 64])        # 2,874 anchors
MID_HEADS = dict(shapes=[(36, 120), (18, 60)], field=[60, 120], ds=[8, 16])                       # 5,400 anchors
FULL_SHAPES = [(72, 240), (72, 240), (36, 120), (36, 120), (18, 60), (18, 60), (9, 30)]           # 7s-576: 45,630 anchors
CALTECH = dict(shapes=[(60, 80), (60, 80), (30, 40), (30, 40), (15, 20), (15, 20), (8, 10)],       # 480 x 640: 12,680 anchors
               field_w=[20, 28, 40, 56, 80, 112, 160], field_h=[40, 56, 80, 112, 160, 224, 320], ds=[8, 8, 16, 16, 32, 32, 64])
DENSE, SPARSE, EMPTY = -8.0, 6.0, 60.0          # background bias of an image: nearly every anchor / a part / none passes fg_thr
GUARD = 64                                      # rows behind `cap` that no op may touch
F_SENT, I_SENT = -12345.0, -777


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X: torch.cuda.is_available() is False")
    from mscnn_amd import hipapi
    hipapi.lib()
    return hipapi


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_heads(seed, shapes, biases, cls=5, sigma=2.0):
    """One (num, cls + 4, h, w) array per head; image i has background bias biases[i] (test_gpu_ops._heads, per image)."""
    rng = np.random.default_rng(seed)
    out = []
    for (h, w) in shapes:
        t = rng.standard_normal((len(biases), cls + 4, h, w)).astype(np.float32)
        t[:, :cls] *= sigma
        t[:, 0] += np.asarray(biases, np.float32)[:, None, None]
        t[:, cls:] *= 0.5
        out.append(t)
    return out


class Op:
    """One form of the op on buffers filled with sentinels, with a guard band behind them and a workspace full of garbage."""

    def __init__(self, hip, d, one_pass, cap=None, props=True, aids=True):
        L = hip.lib()
        self.L, self.d, self.one_pass = L, d, one_pass
        self.cap = cap if cap is not None else L.mscnn_boxoutput_max_rows(C.byref(d))
        wb = (L.mscnn_boxoutput_batch_workspace_bytes if one_pass else L.mscnn_boxoutput_workspace_bytes)(C.byref(d))
        assert wb > 0, L.mscnn_last_error()
        self.ws = torch.full((wb,), 0xA5, dtype=torch.uint8, device="cuda")
        self.want_props, self.want_aids = props, aids

    def __call__(self, heads):
        n = self.cap + GUARD
        rois = torch.full((n, 5), F_SENT, dtype=torch.float32, device="cuda")
        props = torch.full((n, 6), F_SENT, dtype=torch.float32, device="cuda")
        aids = torch.full((n,), I_SENT, dtype=torch.int32, device="cuda")
        count = torch.full((2 + GUARD,), I_SENT, dtype=torch.int32, device="cuda")
        ptrs = (C.c_void_p * len(heads))(*[h.data_ptr() for h in heads])
        fwd = self.L.mscnn_boxoutput_batch_fwd_f32 if self.one_pass else self.L.mscnn_boxoutput_fwd_f32
        rc = fwd(C.byref(self.d), ptrs, rois.data_ptr(), props.data_ptr() if self.want_props else None,
                 aids.data_ptr() if self.want_aids else None, self.cap, count.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, self.L.mscnn_last_error()
        torch.cuda.synchronize()
        return rois.cpu().numpy(), props.cpu().numpy(), aids.cpu().numpy(), count.cpu().numpy()


def same_words(got, want):
    for g, w, what in zip(got, want, ("rois", "props", "anchor ids", "count")):
        assert np.array_equal(g, w), what


def check(hip, orc, heads, geom, num, cls=5, oracle=True, cap=None, props=True, aids=True, **kw):
    """one-pass == per-image op on every word (guard band and unwritten rows included) == the oracle's rows.
    Returns (R, real rows, rows per image)."""
    fw, fh = geom.get("field_w", geom.get("field")), geom.get("field_h", geom.get("field"))
    d = hip.make_boxoutput_desc(geom["shapes"], num, cls + 4, fw, fh, geom["ds"], **kw)
    hd = [dev(h) for h in heads]
    one = Op(hip, d, True, cap, props, aids)(hd)
    per = Op(hip, d, False, cap, props, aids)(hd)
    same_words(one, per)
    rois, prp, ids, count = one
    R, real = int(count[0]), int(count[1])
    assert np.all(count[2:] == I_SENT)                                  # two count words, nothing behind them
    w = min(R, rois.shape[0] - GUARD)                                   # rows written: the first `cap` of the R
    assert np.all(rois[w:] == F_SENT) and np.all(prp[w if props else 0:] == F_SENT) and np.all(ids[w if aids else 0:] == I_SENT)
    if oracle:
        ref = orc.boxoutput(heads, fw, fh, geom["ds"], with_anchor_ids=True, **kw)
        assert R == ref[0].shape[0] and real == ref[3]
        assert np.array_equal(rois[:w], ref[0][:w])
        if props:
            assert np.array_equal(prp[:w], ref[1][:w])
        if aids:
            assert np.array_equal(ids[:w], ref[4][:w])
    img = rois[:w, 0].astype(int)
    assert np.all(np.diff(img) >= 0)                                    # grouped by image, in image order
    return R, real, np.bincount(img, minlength=num) if real else np.zeros(num, int)


KW = dict(fg_thr=-5.0, iou_thr=0.65, max_nms_num=2000, min_size=15.0)


@pytest.mark.parametrize("B", [1, 2, 3, 8, 35])
def test_batch_sizes(hip, orc, B):
    """B images of alternating regimes; 35 runs as a group of 32 and a group of 3 with the row offset carried over."""
    biases = [(DENSE, SPARSE, -2.0)[i % 3] for i in range(B)]
    R, real, per_image = check(hip, orc, make_heads(100 + B, KITTI_HEADS["shapes"], biases), KITTI_HEADS, B, **KW)
    assert R == real and per_image.min() > 0


@pytest.mark.parametrize("name,biases", [
    ("empty_first", [EMPTY, DENSE, SPARSE, DENSE]), ("empty_middle", [DENSE, EMPTY, EMPTY, SPARSE]),
    ("empty_last", [SPARSE, DENSE, EMPTY]), ("all_empty", [EMPTY, EMPTY, EMPTY]),
])
def test_mixed_regimes_and_empty_images(hip, orc, name, biases):
    """dense, sparse, truncated (max_nms_num 300 cuts the candidate list of the dense images) and empty images in one batch"""
    kw = dict(KW, max_nms_num=300)
    R, real, per_image = check(hip, orc, make_heads(7, KITTI_HEADS["shapes"], biases), KITTI_HEADS, len(biases), **kw)
    if name == "all_empty":
        assert (R, real) == (1, 0)                                      # the single dummy row of the batch
    else:
        assert R == real and [n > 0 for n in per_image] == [b != EMPTY for b in biases]


def test_all_empty_dummy_row_words(hip):
    d = hip.make_boxoutput_desc(KITTI_HEADS["shapes"], 3, 9, KITTI_HEADS["field"], KITTI_HEADS["field"], KITTI_HEADS["ds"], **KW)
    heads = [dev(h) for h in make_heads(8, KITTI_HEADS["shapes"], [EMPTY] * 3)]
    rois, props, aids, count = Op(hip, d, True)(heads)
    assert rois[0].tolist() == [0, 1, 1, 10, 10] and props[0].tolist() == [0] * 6 and aids[0] == -1 and count[:2].tolist() == [1, 0]


def test_max_post_nms_num_binds_on_some_images(hip, orc):
    heads = make_heads(9, KITTI_HEADS["shapes"], [DENSE, 11.0, DENSE, 14.0])
    _, _, free = check(hip, orc, heads, KITTI_HEADS, 4, **KW)
    post = int(np.sort(free)[1:3].mean())                              # between the sparse images' rows and the dense images'
    assert free.min() < post < free.max()
    _, _, cut = check(hip, orc, heads, KITTI_HEADS, 4, max_post_nms_num=post, **KW)
    assert cut.tolist() == [min(n, post) for n in free]


@pytest.mark.parametrize("K", [1024, 3000, 4032])
def test_k_bounds_on_the_reduced_heads(hip, orc, K):
    """K = 1024 binds; 3000 and 4032 are bounded by the 2,874 anchors (a 4096-key network either way)"""
    check(hip, orc, make_heads(K, KITTI_HEADS["shapes"], [DENSE, DENSE, SPARSE]), KITTI_HEADS, 3, **dict(KW, max_nms_num=K))


@pytest.mark.parametrize("K", [3000, 4032])
def test_k_bounds_that_bind(hip, orc, K):
    R, _, per_image = check(hip, orc, make_heads(K, MID_HEADS["shapes"], [DENSE, -1.0]), MID_HEADS, 2, **dict(KW, max_nms_num=K))
    assert per_image.min() > 100


def test_bboxnorm_with_score_plateaus(hip, orc):
    """the ties case of test_gpu_ops.test_boxoutput_batch2_bboxnorm_ties, with a third image"""
    shapes = [(12, 20), (6, 10)]
    heads = make_heads(11, shapes, [-4.0] * 3, cls=3)
    heads[0][1] = heads[0][0]                                   # image 1 == image 0 on head 0
    heads[0][:, 1:3, 4:8, :] = 1.5                              # plateaus of exactly equal scores (tie-break by index)
    kw = dict(fg_thr=-7.0, iou_thr=0.65, max_nms_num=100, min_size=5.0, bbox_mean=[0, 0, 0, 0], bbox_std=[0.1, 0.1, 0.2, 0.2])
    geom = dict(shapes=shapes, field_w=[40, 80], field_h=[56, 112], ds=[8, 16])
    check(hip, orc, heads, geom, 3, cls=3, **kw)


@pytest.mark.parametrize("mode", ["IOU", "IOMU", "IOFU"])
def test_nms_modes(hip, orc, mode):
    check(hip, orc, make_heads(21, KITTI_HEADS["shapes"], [DENSE, -2.0]), KITTI_HEADS, 2, nms_type=mode, **KW)


def test_props_and_anchor_ids_null(hip, orc):
    check(hip, orc, make_heads(22, KITTI_HEADS["shapes"], [DENSE, EMPTY, SPARSE]), KITTI_HEADS, 3, props=False, aids=False, **KW)


def test_cap_below_the_row_total(hip, orc):
    """the counts say what the batch holds, the rows stop at cap: nothing is written at or past it (guard band)"""
    heads = make_heads(23, KITTI_HEADS["shapes"], [DENSE, SPARSE, DENSE])
    R, _, per_image = check(hip, orc, heads, KITTI_HEADS, 3, **KW)
    for cap in (R - 1, int(per_image[0]) + 1, 1):                       # inside the last image, inside the second, one row
        assert check(hip, orc, heads, KITTI_HEADS, 3, cap=cap, **KW)[0] == R


def test_large_path_through_the_batch_entry(hip, orc):
    geom = dict(shapes=[(36, 120), (36, 120), (18, 60)], field=[60, 84, 120], ds=[8, 8, 16])      # 9,720 anchors, max_nms_num 0
    R, _, _ = check(hip, orc, make_heads(78, geom["shapes"], [DENSE, 1.0]), geom, 2, **dict(KW, max_nms_num=0))
    assert R > 4032


def test_full_size_7s576_batch_4(hip, orc):
    heads = make_heads(3, FULL_SHAPES, [DENSE, -1.5, SPARSE, DENSE])
    R, real, per_image = check(hip, orc, heads, dict(KITTI_HEADS, shapes=FULL_SHAPES), 4, oracle=False, **KW)
    assert R == real and per_image.min() > 100


def test_full_size_caltech_batch_8(hip, orc):
    biases = [DENSE, -1.5, SPARSE, EMPTY, DENSE, -3.0, 2.0, DENSE]
    R, real, per_image = check(hip, orc, make_heads(4, CALTECH["shapes"], biases, cls=2), CALTECH, 8, cls=2, oracle=False, **KW)
    assert R == real and [n > 0 for n in per_image] == [b != EMPTY for b in biases]


def test_two_calls_on_one_workspace(hip, orc):
    """different heads through one workspace, back and forth: no state leaks from call to call"""
    d = hip.make_boxoutput_desc(KITTI_HEADS["shapes"], 3, 9, KITTI_HEADS["field"], KITTI_HEADS["field"], KITTI_HEADS["ds"], **KW)
    a = [dev(h) for h in make_heads(31, KITTI_HEADS["shapes"], [DENSE, SPARSE, DENSE])]
    b = [dev(h) for h in make_heads(32, KITTI_HEADS["shapes"], [SPARSE, EMPTY, -2.0])]
    fresh_a, fresh_b = Op(hip, d, False)(a), Op(hip, d, False)(b)
    op = Op(hip, d, True)
    for heads, want in ((a, fresh_a), (b, fresh_b), (b, fresh_b), (a, fresh_a)):
        same_words(op(heads), want)


def test_python_class_one_pass(hip, orc):
    heads = make_heads(41, KITTI_HEADS["shapes"], [DENSE, SPARSE])
    d = hip.make_boxoutput_desc(KITTI_HEADS["shapes"], 2, 9, KITTI_HEADS["field"], KITTI_HEADS["field"], KITTI_HEADS["ds"], **KW)
    ref = orc.boxoutput(heads, KITTI_HEADS["field"], KITTI_HEADS["field"], KITTI_HEADS["ds"], with_anchor_ids=True, **KW)
    rois, props, aids, nreal = hip.BoxOutput(d, one_pass=True).forward([dev(h) for h in heads])
    assert nreal == ref[3] and np.array_equal(rois.cpu().numpy(), ref[0]) and np.array_equal(props.cpu().numpy(), ref[1])
    assert np.array_equal(aids.cpu().numpy(), ref[4])


# ---- the Net: the switch on and off ------------------------------------------------------------------------------------------------
def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _forward(model, size, batch, one_pass):
    n = mnet.Net(prototxt_text=zoo.prototxt(model, batch=batch, **size))
    n.set_boxoutput_one_pass(one_pass)
    synth.load_into(n, "mid")
    N, _, H, W = n.blob_shape("data")
    orgs = [(375 + 25 * i, 1242 - 50 * i) for i in range(N)]
    n.set_blob("data", np.concatenate([synth.frame(H, W, seed=31 + 7 * i, org_hw=orgs[i]) for i in range(N)], 0))
    n.forward()
    return n, [dict(ratios=(H / float(o[0]), W / float(o[1])), org_hw=o) for o in orgs]


def _same_blobs(on, off, blobs):
    for blob in blobs:
        assert on.blob_shape(blob) == off.blob_shape(blob), blob
        a, b = np.ascontiguousarray(on.get_blob(blob), np.float32), np.ascontiguousarray(off.get_blob(blob), np.float32)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), blob


@pytest.mark.parametrize("model,size,batch,classes", [
    ("caltech/mscnn-7s-480", dict(), 4, [2]),
    ("kitti_car/mscnn-7s-576", dict(height=96, width=320, max_nms_num=120), 2, [2]),
])
def test_net_one_pass_on_equals_off(model, size, batch, classes):
    (on, params), (off, _) = _forward(model, size, batch, True), _forward(model, size, batch, False)
    R = on.blob_shape("proposals")[0]
    assert R > batch
    _same_blobs(on, off, ("proposals", "proposals_score", "bbox_pred", "cls_pred"))
    assert set(on.get_blob("proposals").reshape(R, 5)[:, 0].tolist()) == set(float(i) for i in range(batch))
    (s_on, r_on), (s_off, r_off) = on.detect_multi(params, classes), off.detect_multi(params, classes)
    assert r_on == r_off and sum(r_on) == R
    for i in range(batch):
        for c in range(len(classes)):
            assert _same(s_on[i][c][0], s_off[i][c][0]) and np.array_equal(s_on[i][c][1], s_off[i][c][1]), (i, c)


def test_net_cascade_deploy_batch_2_on_equals_off():
    model, size = "kitti_car/cascade-mscnn-7s-576-2x", dict(height=192, width=448, max_nms_num=150)
    (on, _), (off, _) = _forward(model, size, 2, True), _forward(model, size, 2, False)
    assert on.blob_shape("proposals")[0] > 6
    _same_blobs(on, off, list(on.outputs) + ["proposals", "proposals_score"])
