"""The images of ONE batched forward into the lists of the frames they are views of, on the GPU:
mscnn_detections_candidates_add_views / _cascade_add_views + mscnn_detections_merge_fwd through the HIP ABI on synthetic, seeded ROI
blobs (built as tests/test_gpu_detect_merge.py builds them), and Net.set_image_views / detect_merge_add(..., list_of=) on a reduced
deploy.  Everything is compared bit for bit (doubles as uint64, floats as uint32, tags, counts); no tolerance is involved.

The expectation is the numpy witness (tests/views_witness.py over tests/merge_witness.py; no pin on the reference, whose scripts have
neither views nor a merge): a list holds its images in (add call, image index ascending, row) order.  The Net-level case compares with
the witness applied to the blobs of the batched forward ITSELF, never with batch-1 forwards: bit-identity between batch sizes is not
promised."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import merge_witness as mw                       # noqa: E402
import test_gpu_detect_merge as tm               # noqa: E402  (its synthetic blobs and readers; nothing of it is collected from here)
import views_witness as vw                       # noqa: E402
from mscnn_amd import net as mnet, synth, zoo   # noqa: E402

STD = tm.STD
IDENT = (0.0, 0.0, 0)
COMBOS = tm.COMBOS


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X: torch.cuda.is_available() is False")
    from mscnn_amd import hipapi
    hipapi.lib()
    return hipapi


dev = tm.dev
same_bits = tm.same_bits


class Batch:
    """One batched forward: rows per image, and per image its view, the view's size and the ratios of the input size; blobs of the
    plain stage whose boxes are the cluster boxes of tm.boxes_in_frame seen through each image's view."""

    def __init__(self, rows, ncls, views, hws, ratios, seed, k0=0):
        rng = np.random.default_rng(seed)
        self.rows, self.ncls, self.views, self.hws, self.ratios = rows, ncls, views, hws, ratios
        parts = []
        for i, n in enumerate(rows):
            x, y, w, h = tm.boxes_in_frame(n, k0 + i, rng)
            xv, yv = tm.into_view(x, y, w, views[i], hws[i][1])
            r = ratios[i]
            p = np.stack([np.full(n, float(i)), xv * r[1], yv * r[0], (xv + w) * r[1], (yv + h) * r[0], rng.uniform(-1, 1, n)], 1).astype(np.float32)
            if n >= 5:
                p[1, 5] = -11.0                    # under proposal_thr: filtered
                p[2, 3] = p[2, 1]                  # zero width: filtered
            parts.append(p)
        self.props = np.ascontiguousarray(np.concatenate(parts))
        R = len(self.props)
        assert R >= 1
        self.bbox_pred = (rng.standard_normal((R, 4 * ncls)) * 0.3).astype(np.float32)
        self.cls_pred = (rng.standard_normal((R, ncls)) * 2).astype(np.float32)
        self.row0 = np.concatenate([[0], np.cumsum(rows)]).astype(int)

    def segs(self, classes, overlap=0.5):
        return [dict(cls_id=c, bbox_mean=(0, 0, 0, 0), bbox_std=STD, proposal_thr=-10.0, ratios=self.ratios[i], org_hw=self.hws[i], nms_overlap=overlap)
                for i in range(len(self.rows)) for c in classes]

    def witness_rows(self, i, cls_id, thr=None, det_thr=0.0):
        sl = slice(self.row0[i], self.row0[i + 1])
        rows, ids = mw.plain_rows(self.bbox_pred[sl], self.cls_pred[sl], self.props[sl], cls_id, thr=thr, det_thr=det_thr, bbox_stds=STD,
                                  proposal_thr=-10.0, ratios=self.ratios[i], org_hw=self.hws[i])
        return mw.apply_view(rows, self.hws[i][1], self.views[i]), ids + self.row0[i]

    def witness_images(self, cls_id, thr=None, det_thr=0.0):
        return [self.witness_rows(i, cls_id, thr, det_thr) for i in range(len(self.rows))]

    def add_to(self, cand, classes, list_of, nms, overlap=0.5):
        cand.add_views(dev(self.bbox_pred), dev(self.cls_pred), dev(self.props), len(self.rows), self.segs(classes, overlap), list_of,
                       views=self.views, nms=nms)


def main_batch(seed=5):
    """N = 3, rows [300, 0, 70]: image 0 crosses the 256-row step and is a tile at an offset, image 1 is empty, image 2 is mirrored."""
    return Batch([300, 0, 70], 4, [tm.TILE, IDENT, tm.FLIP], [tm.TILE_HW, tm.FRAME, tm.FRAME], [(0.5, 0.75), (1.0, 1.0), (1.5, 1.25)], seed)


def device_lists(hip, cand):
    """Per list of the candidate buffer: (box bits [n, 4] uint64, prob bits [n] uint32, tags [n], wanted, overflow), the first
    min(wanted, cap) slots."""
    counts, boxes, probs, tags = tm.cand_arrays(hip, cand)
    out = []
    for s in range(cand.S):
        wanted, over = (int(v) for v in counts[s])
        n = min(wanted, cand.cap)
        lo = s * cand.cap
        out.append((boxes[32 * lo:32 * (lo + n)].view(np.uint64).reshape(n, 4), probs[4 * lo:4 * (lo + n)].view(np.uint32),
                    tags[4 * lo:4 * (lo + n)].view(np.int32), wanted, over))
    return out


def assert_list_equals(got, rows, tags, what):
    box, prob, tag, wanted, over = got
    assert (wanted, over) == (len(rows), 0), (what, wanted, over, len(rows))
    assert np.array_equal(tag, tags), (what, tag.tolist(), tags.tolist())
    assert np.array_equal(box, np.ascontiguousarray(rows[:, :4]).view(np.uint64)), what
    assert np.array_equal(prob, rows[:, 4].astype(np.float32).view(np.uint32)), what


def assert_merge_equals(got, want, what):
    dets, tags, cands = got
    wd, wp, wr, wc = want[:4]
    assert dets is not None, (what, "overflow", cands)
    pas, row = tm.split_tags(tags)
    assert cands == wc, (what, cands, wc)
    assert np.array_equal(pas, wp) and np.array_equal(row, wr), (what, pas.tolist(), wp.tolist(), row.tolist(), wr.tolist())
    assert same_bits(dets, wd), what


# ---- the batch of the issue: N = 3, list_of = [0, 1, 0], 2 classes ---------------------------------------------------------------------------
@pytest.mark.parametrize("t,dn,thr,det_thr", [c + (None, 0.0) for c in COMBOS] + [("maxg", "min", "median", "median")])
def test_a_batch_of_views_against_the_witness(hip, t, dn, thr, det_thr):
    b = main_batch()
    classes, list_of = [2, 3], [0, 1, 0]
    if thr == "median":      # thresholds that sit on probabilities that occur (strict > and >=)
        probs = np.sort(b.witness_rows(0, 2)[0][:, 4])
        thr, det_thr = float(probs[len(probs) // 3]), float(np.float32(probs[len(probs) // 2]))
    images = {c: b.witness_images(c, thr, det_thr) for c in classes}
    # on the witness's own result: a box of image 2 is suppressed by one of image 0 and the other way round, both have a survivor
    later_by_earlier = earlier_by_later = False
    alive = set()
    for c in classes:
        a_, b_, s_ = mw.cross_pass_facts([images[c][0], images[c][2]], 0.5, t, dn)
        later_by_earlier |= a_; earlier_by_later |= b_; alive |= s_
    assert later_by_earlier, "no box of image 2 is suppressed by one of image 0: the case shows nothing"
    assert earlier_by_later, "no box of image 0 is suppressed by one of image 2: the case shows nothing"
    assert alive == {0, 1}
    cap = sum(b.rows)
    cand = hip.Candidates(2 * len(classes), cap)
    nms = tm.nms_arg(hip, t, dn, thr, det_thr)
    b.add_to(cand, classes, list_of, nms)
    lists = device_lists(hip, cand)
    merged = cand.merge(nms=nms)
    for f in range(2):
        for ci, c in enumerate(classes):
            s = f * len(classes) + ci
            rows, tags = vw.candidate_list([images[c]], [list_of], f)
            assert_list_equals(lists[s], rows, tags, (f, c))
            assert_merge_equals(merged[s], vw.merge_views([images[c]], [list_of], f, 0.5, t, dn), (f, c))
    assert lists[2][3] == lists[3][3] == 0 and len(merged[2][0]) == 0      # frame 1 has the empty image only
    if thr is None:
        assert lists[0][3] > 256 + 30, "image 0 must cross the 256-row step with survivors and image 2 follow it"


# ---- identity list_of: the whole buffer is _add's ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_views,thr", [(False, None), (True, 0.3)])
def test_identity_list_of_leaves_the_buffer_byte_identical_to_add(hip, with_views, thr):
    classes = [2, 3]
    passes = [tm.Pass(0, [257, 64, 0], 4, ratios=(1.5, 1.25), view=tm.FLIP if with_views else None, seed=9),
              tm.Pass(1, [3, 0, 70], 4, ratios=(0.5, 0.75), view=tm.TILE if with_views else None, hw=tm.TILE_HW if with_views else tm.FRAME, seed=9)]
    nms = tm.nms_arg(hip, "maxg", "union", thr, 0.0)
    bufs = []
    for views_form in (False, True):
        cand = hip.Candidates(3 * len(classes), 330)
        cand.buf.fill_(0xFF)
        hip._check(hip.lib().mscnn_detections_candidates_reset(hip._dev(cand.buf), cand.S, cand.cap, hip._stream()))
        for p in passes:
            segs = [p.seg_kw(c) for _ in range(3) for c in classes]
            views = None if p.view is None else [p.view] * 3
            if views_form:
                cand.add_views(dev(p.bbox_pred), dev(p.cls_pred), dev(p.props), 3, segs, [0, 1, 2], views=views, nms=nms)
            else:
                cand.add(dev(p.bbox_pred), dev(p.cls_pred), dev(p.props), 3, segs, views=views, nms=nms)
        bufs.append(cand.buf.cpu().numpy())
        counts = cand.counts()
    assert counts[0][0] > (256 if thr is None else 0) and counts[4][0] > 0 and all(c[1] == 0 for c in counts)
    assert np.array_equal(bufs[0], bufs[1])


# ---- more source segments than one launch's table, a second call, the cap ---------------------------------------------------------------------
def test_34_source_segments_of_one_frame_keep_the_order_image_then_row(hip):
    rows = [5, 3, 6, 4, 0, 5, 6, 3, 4, 5, 6, 7, 2, 5, 0, 6, 9]
    assert len(rows) == 17
    views = [IDENT, tm.FLIP, tm.TILE] * 5 + [IDENT, tm.FLIP]
    hws = [tm.TILE_HW if v is tm.TILE else tm.FRAME for v in views]
    b = Batch(rows, 3, views, hws, [(1.0, 1.0), (1.5, 1.25), (0.5, 0.75)] * 5 + [(1.0, 1.0), (1.5, 1.25)], seed=17)
    classes, list_of = [1, 3], [0] * 17
    cand = hip.Candidates(len(classes), sum(rows))
    b.add_to(cand, classes, list_of, hip.NMS_NULL)
    lists = device_lists(hip, cand)
    merged = cand.merge()
    for ci, c in enumerate(classes):
        images = b.witness_images(c)
        rows_w, tags_w = vw.candidate_list([images], [list_of], 0)
        assert len(rows_w) > 40 and np.all(np.diff(tags_w) > 0), "rows absolute in the batch, ascending: (image, row)"
        assert_list_equals(lists[ci], rows_w, tags_w, c)
        want = vw.merge_views([images], [list_of], 0)
        assert len(set(want[4].tolist())) >= 8, "the images do not all reach the result: the case shows little"
        assert_merge_equals(merged[ci], want, c)


def test_a_second_call_appends_behind_the_first(hip):
    classes = [2]
    first = main_batch(seed=23)
    second = Batch([40, 66], 4, [tm.FLIP, IDENT], [tm.FRAME, tm.FRAME], [(1.25, 1.5), (1.0, 1.0)], seed=24, k0=3)
    lof = [[0, 1, 0], [1, 0]]
    cand = hip.Candidates(2, sum(first.rows) + sum(second.rows))
    first.add_to(cand, classes, lof[0], hip.NMS_NULL)
    second.add_to(cand, classes, lof[1], hip.NMS_NULL)
    adds = [first.witness_images(2), second.witness_images(2)]
    lists = device_lists(hip, cand)
    merged = cand.merge()
    for f in range(2):
        rows, tags = vw.candidate_list(adds, lof, f)
        assert_list_equals(lists[f], rows, tags, f)
        assert_merge_equals(merged[f], vw.merge_views(adds, lof, f), f)
    assert set((lists[0][2] >> 24).tolist()) == {0, 1} and set((lists[1][2] >> 24).tolist()) == {1}
    n_first = len(vw.candidate_list(adds[:1], lof[:1], 0)[0])
    assert np.all(lists[0][2][:n_first] >> 24 == 0) and np.all(lists[0][2][n_first:] >> 24 == 1)


def test_a_cap_one_below_the_rows_that_want_in(hip):
    """Frame 0's list would hold the kept rows of images 0 and 2; with one slot less the overflow flag is set, the count keeps running
    and nothing is stored past the cap (the buffer was poison before the reset); frame 1's list, untouched by it, is as it was."""
    classes, list_of = [2], [0, 1, 0]
    b = Batch([300, 10, 70], 4, [tm.TILE, IDENT, tm.FLIP], [tm.TILE_HW, tm.FRAME, tm.FRAME], [(0.5, 0.75), (1.0, 1.0), (1.5, 1.25)], seed=31)
    images = b.witness_images(2)
    full = len(images[0][0]) + len(images[2][0])
    few = len(images[1][0])
    assert full > 300 and 0 < few <= 10 and len(images[2][0]) > 1
    for cap, over in ((full, False), (full - 1, True)):
        cand = hip.Candidates(2, cap)
        cand.buf.fill_(0xFF)
        hip._check(hip.lib().mscnn_detections_candidates_reset(hip._dev(cand.buf), 2, cap, hip._stream()))
        b.add_to(cand, classes, list_of, hip.NMS_NULL)
        counts, boxes, probs, tags = tm.cand_arrays(hip, cand)
        assert counts.tolist() == [[full, int(over)], [few, 0]]
        stored = [min(full, cap), few]
        for arr, item in ((boxes, 32), (probs, 4), (tags, 4)):
            used = np.zeros(len(arr), bool)
            for s in range(2):
                used[item * s * cap:item * (s * cap + stored[s])] = True
            assert np.all(arr[~used] == 0xFF), "a byte outside the stored slots was written"
            assert not np.all(arr[used] == 0xFF)
        rows, tg = vw.candidate_list([images], [list_of], 0)
        assert np.array_equal(tags[:4 * stored[0]].view(np.int32), tg[:stored[0]])      # what fits is stored, in order
        merged = cand.merge()
        assert_merge_equals(merged[1], vw.merge_views([images], [list_of], 1), "frame 1")
        if over:
            assert merged[0] == (None, None, full)
        else:
            assert_merge_equals(merged[0], vw.merge_views([images], [list_of], 0), "frame 0")


# ---- the cascade form ---------------------------------------------------------------------------------------------------------------------------
def test_cascade_views_against_the_witness(hip):
    rows, classes, O, list_of = [65, 40, 33], [2], 2, [0, 1, 0]
    ratios, view = (1.5, 1.25), tm.FLIP
    outs = tm.cascade_pass(0, rows, O, 2, view=view, ratios=ratios, seed=19)
    segs = [dict(cls_id=c, ratios=ratios, org_hw=tm.FRAME, nms_overlap=0.5) for _ in rows for _ in range(O) for c in classes]
    cand = hip.Candidates(2 * O * len(classes), sum(rows))
    cand.cascade_add_views([tuple(dev(b) for b in o) for o in outs], 3, segs, list_of, det_thr=0.1, views=[view] * 3)
    lists = device_lists(hip, cand)
    merged = cand.merge()
    row0 = [0, 65, 105, 138]
    total = 0
    for f in range(2):
        for o in range(O):
            boxes, prob, props = outs[o]
            images = []
            for i in range(3):
                sl = slice(row0[i], row0[i + 1])
                r, ids = mw.cascade_rows(boxes[sl], prob[sl], props[sl], 2, ratios=ratios, org_hw=tm.FRAME, det_thr=0.1)
                images.append((mw.apply_view(r, tm.FRAME[1], view), ids + row0[i]))
            s = f * O + o
            rows_w, tags_w = vw.candidate_list([images], [list_of], f)
            assert_list_equals(lists[s], rows_w, tags_w, (f, o))
            want = vw.merge_views([images], [list_of], f)
            assert_merge_equals(merged[s], want, (f, o))
            if f == 0:
                assert set(want[4].tolist()) == {0, 1}, "both images of frame 0 must have a survivor"
            total += len(want[0])
    assert total > 20


# ---- Net level ----------------------------------------------------------------------------------------------------------------------------------
def test_net_tiles_and_their_mirrors_as_one_batched_forward(hip):
    kw = dict(height=96, width=320, max_nms_num=200)
    text = zoo.prototxt("kitti_car/mscnn-7s-576", **kw)
    n = mnet.Net(prototxt_text=text)
    synth.load_into(n, "mid")
    fresh = mnet.Net(prototxt_text=text)
    synth.load_into(fresh, "mid")
    # a 120 x 400 frame: the seeded KITTI-shaped frame (rectangles on low-pass noise) scaled down, as uint8 RGB
    x = synth.frame(120, 400, seed=47)[0].transpose(1, 2, 0)[:, :, ::-1] + np.array([123.0, 117.0, 104.0])
    img = np.ascontiguousarray(np.clip(np.round(x), 0, 255).astype(np.uint8))
    classes = [2, 3]
    views, _, mviews = mnet.tile_views((120, 400), rows=1, cols=2, overlap=40, flip=True)
    N = len(views)
    assert N == 4
    n.reshape_input("data", (N, 3, 96, 320))
    params = n.set_image_views("data", [img], views)
    assert params == [dict(ratios=(96 / 120.0, 320 / 220.0), org_hw=(120, 220))] * 4
    blob = n.get_blob("data")
    for v in range(N):      # the input blob: set_image on each host crop, bit for bit
        fresh.set_image("data", vw.crop(img, views[v]))
        assert np.array_equal(blob[v:v + 1], fresh.get_blob("data")), v
    dev_params = n.set_image_views("data", [torch.from_numpy(img).cuda()], views)      # a device frame: the same blob
    assert dev_params == params and np.array_equal(n.get_blob("data"), blob)
    n.forward()
    R = n.blob_shape("proposals_score")[0]
    n.detect_merge_begin(1, len(classes), R)
    with pytest.raises(mnet.NetError, match=r"image 2: list_of 1 outside \[0, 1\): the merge was begun with 1 frames"):
        n.detect_merge_add(params, classes, views=mviews, list_of=[0, 0, 1, 0])
    with pytest.raises(mnet.NetError, match="begun with 1 images but the net's input holds 4"):      # without list_of: the call it always was
        n.detect_merge_add(params, classes, views=mviews)
    n.detect_merge_add(params, classes, views=mviews, list_of=[0] * N)
    with pytest.raises(mnet.NetError, match=f"{R} ROI rows, this one {R}: more than cand_cap {R}"):
        n.detect_merge_add(params, classes, views=mviews, list_of=[0] * N)
    per_image, cands = n.detect_merge_end()
    blobs = [n.get_blob(b).reshape(R, -1) for b in ("bbox_pred", "cls_pred", "proposals_score")]
    image_of = blobs[2][:, 0].astype(int)
    assert np.all(np.diff(image_of) >= 0)
    total, contributing = 0, set()
    for ci, c in enumerate(classes):
        images = []
        for b in range(N):
            idx = np.flatnonzero(image_of == b)
            rows, ids = mw.plain_rows(*[x[idx] for x in blobs], c, bbox_stds=STD, proposal_thr=-10.0, ratios=params[b]["ratios"],
                                      org_hw=params[b]["org_hw"])
            view = (mviews[b]["off_x"], mviews[b]["off_y"], mviews[b]["flip_x"])
            images.append((mw.apply_view(rows, params[b]["org_hw"][1], view), ids + (idx[0] if len(idx) else 0)))
        wd, wp, wr, wc, wimg = vw.merge_views([images], [[0] * N], 0)
        dets, pas, row = per_image[0][ci]
        assert cands[0][ci] == wc and np.array_equal(pas, wp) and np.array_equal(row, wr) and same_bits(dets, wd), c
        assert np.all(pas == 0), "one batched forward is one pass"
        total += len(dets)
        contributing |= set(wimg.tolist())
    assert total > 3 and len(contributing) >= 2, "the views do not interact on this net: the case shows nothing"
    # nothing is left behind: a plain forward + detect_multi afterwards is a fresh net's, bit for bit
    res = []
    for net in (n, fresh):
        net.reshape_input("data", (1, 3, 96, 320))
        p = net.set_images("data", [img])
        net.forward()
        res.append(net.detect_multi(p, classes))
    assert res[0][1] == res[1][1]
    for ci in range(len(classes)):
        assert same_bits(res[0][0][0][ci][0], res[1][0][0][ci][0]) and np.array_equal(res[0][0][0][ci][1], res[1][0][0][ci][1])
