"""Several forwards of an image, one NMS, on the GPU: mscnn_detections_candidates_add / _cascade_add + mscnn_detections_merge_fwd
through the HIP ABI on synthetic, seeded ROI blobs, and Net.detect_merge_* on reduced deploys.  Everything is compared bit for bit
(doubles as uint64, tags, counts, table words); no tolerance is involved.

Two kinds of expectation:
  * invariants against ops that are pinned elsewhere: one add + merge is mscnn_detections_multi_nms_fwd (resp. the cascade call) on
    the same blobs, and the same forward added twice is that result again with pass 0 in every tag;
  * the numpy witness (tests/merge_witness.py; no pin on the reference, whose scripts run one forward per image).  Each witness case
    first shows ON THE WITNESS'S OWN RESULT that a box of a later pass is suppressed by one of an earlier pass, one of an earlier pass
    by one of a later pass, and that every pass has a survivor -- a case can not pass without cross-pass interaction."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import guarded                                   # noqa: E402
import merge_witness as mw                       # noqa: E402
from mscnn_amd import net as mnet, synth, zoo   # noqa: E402

INF = float("inf")
STD = (0.1, 0.1, 0.2, 0.2)
FRAME = (1800, 1600)                     # (H, W) of the original image every synthetic case lives in
FLIP = (0.0, 0.0, 1)
TILE = (37.5, 20.25, 0)                  # a view whose corner lies at (37.5, 20.25) of the frame ...
TILE_HW = (1700, 1000)                   # ... 1000 wide: the clusters at x >= 1000 are clipped to zero / negative widths in it
COMBOS = [("maxg", "union"), ("maxg", "min"), ("max", "union"), ("max", "min")]


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X: torch.cuda.is_available() is False")
    from mscnn_amd import hipapi
    hipapi.lib()
    return hipapi


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def split_tags(tags):
    tags = np.asarray(tags, np.int32)
    return tags >> 24, tags & 0xffffff


# ---- synthetic passes ---------------------------------------------------------------------------------------------------------------------
def boxes_in_frame(n, k, rng):
    """n boxes [x y w h] in frame coordinates: members of 8 clusters every pass and image shares (so boxes of different passes
    overlap), row 0 alone at a place of the pass's own (so every pass with a row has a survivor)."""
    m = rng.integers(0, 8, n)
    x = 100 + 300 * (m % 4) + rng.integers(-10, 11, n)
    y = 100 + 300 * (m // 4) + rng.integers(-10, 11, n)
    w = rng.choice([14, 20, 32, 48], n)
    h = rng.choice([14, 20, 32, 48], n)
    if n:
        x[0], y[0], w[0], h[0] = 100 + 150 * k, 1500, 20, 20
    return x.astype(np.float64), y.astype(np.float64), w.astype(np.float64), h.astype(np.float64)


def into_view(x, y, w, view, view_w):
    """Frame coordinates -> the view's: the inverse of the view formula (offset off, then mirrored)."""
    if view is None:
        return x, y
    ox, oy, flip = view
    xv, yv = x - ox, y - oy
    return (view_w - (xv + w) if flip else xv), yv


class Pass:
    """One forward: rows per image, the ratios of its input size, its view and the view's size; blobs of the plain stage."""

    def __init__(self, k, rows, ncls, ratios=(1.0, 1.0), view=None, hw=FRAME, seed=0):
        rng = np.random.default_rng(1000 * seed + k)
        self.k, self.rows, self.ratios, self.view, self.hw, self.ncls = k, rows, ratios, view, hw, ncls
        parts = []
        for i, n in enumerate(rows):
            x, y, w, h = boxes_in_frame(n, k, rng)
            xv, yv = into_view(x, y, w, view, hw[1])
            p = np.stack([np.full(n, float(i)), xv * ratios[1], yv * ratios[0], (xv + w) * ratios[1], (yv + h) * ratios[0],
                          rng.uniform(-1, 1, n)], 1).astype(np.float32)
            if n >= 5:
                p[1, 5] = -11.0                    # under proposal_thr: filtered
                p[2, 3] = p[2, 1]                  # zero width: filtered
            parts.append(p)
        self.props = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros((0, 6), np.float32)
        R = len(self.props)
        if R == 0:                                 # (BoxOutput emits at least one row: an all-zero one when nothing survives)
            self.props = np.zeros((1, 6), np.float32)
            R = 1
        self.bbox_pred = (rng.standard_normal((R, 4 * ncls)) * 0.3).astype(np.float32)
        self.cls_pred = (rng.standard_normal((R, ncls)) * 2).astype(np.float32)
        self.row0 = np.concatenate([[0], np.cumsum(rows)]).astype(int)
        if sum(rows) == 0:
            self.row0 = np.concatenate([[0], np.cumsum([1] + list(rows[1:]))]).astype(int)

    def seg_kw(self, cls_id, overlap=0.5):
        return dict(cls_id=cls_id, bbox_mean=(0, 0, 0, 0), bbox_std=STD, proposal_thr=-10.0, ratios=self.ratios, org_hw=self.hw, nms_overlap=overlap)

    def witness_rows(self, i, cls_id, thr=None, det_thr=0.0):
        sl = slice(self.row0[i], self.row0[i + 1])
        rows, ids = mw.plain_rows(self.bbox_pred[sl], self.cls_pred[sl], self.props[sl], cls_id, thr=thr, det_thr=det_thr, bbox_stds=STD,
                                  proposal_thr=-10.0, ratios=self.ratios, org_hw=self.hw)
        return mw.apply_view(rows, self.hw[1], self.view), ids + self.row0[i]

    def add_to(self, cand, classes, nms, overlap=0.5):
        B = len(self.rows)
        segs = [self.seg_kw(c, overlap) for _ in range(B) for c in classes]
        cand.add(dev(self.bbox_pred), dev(self.cls_pred), dev(self.props), B, segs, views=None if self.view is None else [self.view] * B, nms=nms)


def nms_arg(hip, t, dn, thr=None, det_thr=0.0):
    return hip.NMS_NULL if (t, dn, thr, det_thr) == ("maxg", "union", None, 0.0) else dict(type=t, ovr_dnm=dn, thr=thr, det_thr=det_thr)


def witness_case(passes, classes, overlap=0.5, t="maxg", dn="union", thr=None, det_thr=0.0):
    """[(dets, pass, row, candidates)] per segment, image-major then class, and the cross-pass facts over all segments."""
    B = len(passes[0].rows)
    out, later_by_earlier, earlier_by_later, alive = [], False, False, set()
    for i in range(B):
        for c in classes:
            lists = [p.witness_rows(i, c, thr, det_thr) for p in passes]
            out.append(mw.merge(lists, overlap, t, dn))
            if sum(len(r) for r, _ in lists):
                a, b, s = mw.cross_pass_facts(lists, overlap, t, dn)
                later_by_earlier |= a; earlier_by_later |= b; alive |= s
    return out, (later_by_earlier, earlier_by_later, alive)


def device_case(hip, passes, classes, cap, overlap=0.5, nms=None, **merge_kw):
    B = len(passes[0].rows)
    cand = hip.Candidates(B * len(classes), cap)
    for p in passes:
        p.add_to(cand, classes, hip.NMS_NULL if nms is None else nms, overlap)
    return cand, cand.merge(nms=hip.NMS_NULL if nms is None else nms, **merge_kw)


def assert_equals_witness(got, want, what=""):
    assert len(got) == len(want)
    for s, ((dets, tags, cands), (wd, wp, wr, wc)) in enumerate(zip(got, want)):
        assert dets is not None, (what, s, "overflow", cands)
        pas, row = split_tags(tags)
        assert cands == wc, (what, s, cands, wc)
        assert np.array_equal(pas, wp) and np.array_equal(row, wr), (what, s, pas.tolist(), wp.tolist(), row.tolist(), wr.tolist())
        assert same_bits(dets, wd), (what, s)


CASES = {
    # rows per image and pass from {0, 1, 63, 64, 65, 256, 257}: one under, on and over the ballot (64) and the step (256)
    "S1_two_passes": (dict(classes=[2], ncls=2), [dict(rows=[257], ratios=(1.5, 1.5)), dict(rows=[256], ratios=(1.0, 1.25), view=FLIP)]),
    "S1_three_passes": (dict(classes=[2], ncls=2), [dict(rows=[65], ratios=(1.0, 1.0)), dict(rows=[1], ratios=(0.5, 0.75), view=TILE, hw=TILE_HW),
                                                    dict(rows=[64], ratios=(1.25, 1.5), view=FLIP)]),
    "S4_an_image_without_rows": (dict(classes=[2, 3], ncls=4), [dict(rows=[257, 64], ratios=(1.5, 1.5)), dict(rows=[63, 0], ratios=(1.0, 1.25), view=FLIP),
                                                                dict(rows=[65, 256], ratios=(0.75, 0.5), view=TILE, hw=TILE_HW)]),
    "S33_across_the_launch_boundary": (dict(classes=[1, 2, 3], ncls=3), [dict(rows=[5, 3, 6, 4, 0, 5, 6, 3, 4, 5, 6], ratios=(1.0, 1.0)),
                                                                         dict(rows=[4, 6, 3, 5, 6, 0, 4, 5, 6, 3, 5], ratios=(1.5, 1.25), view=FLIP),
                                                                         dict(rows=[6, 5, 4, 3, 5, 6, 0, 6, 5, 4, 3], ratios=(0.5, 0.5), view=TILE, hw=TILE_HW)]),
}


def make_passes(name):
    top, specs = CASES[name]
    return top["classes"], [Pass(k, ncls=top["ncls"], seed=7 + len(name), **spec) for k, spec in enumerate(specs)]


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("t,dn", [("maxg", "union"), ("max", "min")])
def test_passes_against_the_witness(hip, name, t, dn):
    classes, passes = make_passes(name)
    want, (later_by_earlier, earlier_by_later, alive) = witness_case(passes, classes, 0.5, t, dn)
    assert later_by_earlier, "no box of a later pass is suppressed by one of an earlier pass: the case shows nothing"
    assert earlier_by_later, "no box of an earlier pass is suppressed by one of a later pass: the case shows nothing"
    assert alive == set(range(len(passes))), alive
    cap = sum(max(p.rows) for p in passes)
    cand, got = device_case(hip, passes, classes, cap, nms=nms_arg(hip, t, dn))
    assert_equals_witness(got, want, name)
    counts = cand.counts()
    assert [c[0] for c in counts] == [w[3] for w in want] and all(c[1] == 0 for c in counts)
    assert len(got) in (1, 4, 33)


def test_thresholds_are_applied_by_the_add_calls(hip):
    """bbNms's thr (strict) and the plain det_thr (>=) sit on probabilities that occur: the witness drops those rows before the merge,
    the add kernels (det_row<true>) must too -- the merge is given the setting but reads type and ovr_dnm only."""
    classes, passes = make_passes("S1_two_passes")
    rows, _ = passes[0].witness_rows(0, 2)
    probs = np.sort(rows[:, 4])
    thr, det_thr = float(probs[len(probs) // 3]), float(np.float32(probs[len(probs) // 2]))
    assert float(np.float32(det_thr)) == det_thr
    want, facts = witness_case(passes, classes, 0.5, "maxg", "min", thr=thr, det_thr=det_thr)
    assert facts[0] and facts[1] and want[0][3] < sum(len(p.witness_rows(0, 2)[0]) for p in passes)
    _, got = device_case(hip, passes, classes, 600, nms=nms_arg(hip, "maxg", "min", thr, det_thr))
    assert_equals_witness(got, want)


# ---- invariants against the pinned single-forward ops -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("t,dn,thr,det_thr", [c + (None, 0.0) for c in COMBOS] + [("maxg", "union", 0.2, 0.3), ("max", "min", 0.25, 0.0)])
def test_one_add_and_merge_equals_the_one_pass_stage_and_twice_added_too(hip, t, dn, thr, det_thr):
    p = Pass(0, [257, 64], 4, ratios=(576 / 375.0, 1920 / 1242.0), hw=(375, 1242), seed=3)
    # (scaled into the 375 x 1242 image, no box clipped: a box of zero or negative extent overlaps nothing in bbNms, its own twin of
    # the second add included, so only boxes with an area make "twice added = once added" true)
    p.props[:, 1:5] *= 0.2
    classes = [2, 3]
    nms = nms_arg(hip, t, dn, thr, det_thr)
    segs = [p.seg_kw(c) for _ in range(2) for c in classes]
    ref = hip.detections_multi(dev(p.bbox_pred), dev(p.cls_pred), dev(p.props), 2, segs, max_rows_per_image=257,
                               nms=None if nms is hip.NMS_NULL else nms)
    assert sum(len(r[0]) for r in ref) > 20
    cand, once = device_case(hip, [p], classes, 257, nms=nms)
    cand2, twice = device_case(hip, [p, p], classes, 2 * 257, nms=nms)
    assert all(np.all(rd[:, 2:4] > 0) for rd, _, _, _ in ref)
    for s, ((rd, rid, row0, rows), (d1, t1, c1), (d2, t2, c2)) in enumerate(zip(ref, once, twice)):
        assert (row0, rows) == ([0, 257][s // 2], [257, 64][s // 2])
        assert same_bits(d1, rd) and np.array_equal(t1, rid + row0), (s, "one add")
        assert same_bits(d2, rd) and np.array_equal(t2, rid + row0), (s, "the same forward twice: every tag from pass 0")
        assert c2 == 2 * c1 and len(rd) <= c1 <= rows


def cascade_pass(k, rows, num_outputs, ncls, view=None, hw=FRAME, ratios=(1.0, 1.0), seed=0):
    """[(boxes [R, 5], cls_prob [R, ncls], props [R, 5])] per cascade output for one forward: the decoded boxes are the cluster boxes of
    boxes_in_frame in the view's net coordinates ([x1 y1 x2 y2], x2 = x1 + w - 1), a zero-width proposal per image."""
    rng = np.random.default_rng(5000 * seed + k)
    outs = []
    for o in range(num_outputs):
        parts = []
        for i, n in enumerate(rows):
            x, y, w, h = boxes_in_frame(n, k, rng)
            xv, yv = into_view(x, y, w + 1, view, hw[1])      # (the cascade rows come out w + 1 wide in original pixels at ratio 1)
            parts.append(np.stack([np.full(n, float(i)), xv * ratios[1], yv * ratios[0], (xv + w) * ratios[1], (yv + h) * ratios[0]], 1))
        boxes = np.ascontiguousarray(np.concatenate(parts).astype(np.float32))
        props = boxes.copy()
        for r0 in np.cumsum([0] + list(rows[:-1])):
            if r0 + 3 < len(props):
                props[r0 + 3, 3] = props[r0 + 3, 1] - 1          # cw = x2 - x1 + 1 = 0: dropped
        p = rng.uniform(0.02, 0.98, (len(boxes), ncls)).astype(np.float32)
        outs.append((boxes, p, props))
    return outs


@pytest.mark.parametrize("t,dn,thr,det_thr", [("maxg", "union", None, 0.0), ("max", "min", 0.3, 0.25)])
def test_cascade_add_and_merge_equals_the_cascade_one_pass_stage(hip, t, dn, thr, det_thr):
    rows, classes, O = [65, 40], [1, 2], 2
    outs = cascade_pass(0, rows, O, 2, seed=11)
    d_outs = [tuple(dev(b) for b in o) for o in outs]
    nms = nms_arg(hip, t, dn, thr, 0.0)
    # (no box is clipped to a zero or negative extent: such a box overlaps nothing, its twin of the second add included)
    segs = [dict(cls_id=c, ratios=(1.25, 1.5), org_hw=(1400, 1000), nms_overlap=0.5) for _ in range(2) for _ in range(O) for c in classes]
    ref = hip.detections_cascade_multi(d_outs, 2, segs, det_thr=det_thr, max_rows_per_image=65, nms=None if nms is hip.NMS_NULL else nms)
    assert sum(len(r[0]) for r in ref) > 20 and all(np.all(r[0][:, 2:4] > 0) for r in ref)
    S = len(segs)
    once = hip.Candidates(S, 65)
    once.cascade_add(d_outs, 2, segs, det_thr=det_thr, nms=nms)
    twice = hip.Candidates(S, 130)
    for _ in range(2):
        twice.cascade_add(d_outs, 2, segs, det_thr=det_thr, nms=nms)
    for s, ((rd, rid, row0, nrows), (d1, t1, c1), (d2, t2, c2)) in enumerate(zip(ref, once.merge(nms=nms), twice.merge(nms=nms))):
        assert (row0, nrows) == ([0, 65][s // 4], rows[s // 4])
        assert same_bits(d1, rd) and np.array_equal(t1, rid + row0), s
        assert same_bits(d2, rd) and np.array_equal(t2, rid + row0) and c2 == 2 * c1, s


def test_cascade_passes_against_the_witness(hip):
    """Two cascade outputs, two images, a plain and a mirrored forward at different ratios: the rows keep w = x2 - x1 + 1 and go
    through the same view formula."""
    rows, classes, O = [64, 33], [2], 2
    specs = [dict(view=None, ratios=(1.0, 1.0)), dict(view=FLIP, ratios=(1.5, 1.25)), dict(view=TILE, hw=TILE_HW, ratios=(0.5, 0.75))]
    fw = [cascade_pass(k, rows, O, 2, seed=13, **sp) for k, sp in enumerate(specs)]
    S = 2 * O * len(classes)
    cand = hip.Candidates(S, 3 * 64)
    for k, sp in enumerate(specs):
        hw = sp.get("hw", FRAME)
        segs = [dict(cls_id=c, ratios=sp["ratios"], org_hw=hw, nms_overlap=0.5) for _ in range(2) for _ in range(O) for c in classes]
        cand.cascade_add([tuple(dev(b) for b in o) for o in fw[k]], 2, segs, det_thr=0.1, views=None if sp["view"] is None else [sp["view"]] * 2)
    got = cand.merge()
    row0 = [0, 64, 97]
    later_by_earlier = earlier_by_later = False
    alive = set()
    for s in range(S):
        i, o, c = s // 2, s % 2, classes[0]
        lists = []
        for k, sp in enumerate(specs):
            boxes, prob, props = fw[k][o]
            sl = slice(row0[i], row0[i + 1])
            hw = sp.get("hw", FRAME)
            r, ids = mw.cascade_rows(boxes[sl], prob[sl], props[sl], c, ratios=sp["ratios"], org_hw=hw, det_thr=0.1)
            lists.append((mw.apply_view(r, hw[1], sp["view"]), ids + row0[i]))
        a, b, al = mw.cross_pass_facts(lists)
        later_by_earlier |= a; earlier_by_later |= b; alive |= al
        assert_equals_witness([got[s]], [mw.merge(lists)], f"cascade segment {s}")
    assert later_by_earlier and earlier_by_later and alive == {0, 1, 2}


# ---- boundaries -------------------------------------------------------------------------------------------------------------------------------
def cand_arrays(hip, cand):
    """The candidate buffer as the header lays it out: (counts [S, 2], boxes [S * cap, 4] + padding, probs, tags) as numpy arrays,
    each WITH the padding up to its 256-byte boundary."""
    S, cap = cand.S, cand.cap
    h = cand.buf.cpu().numpy()
    al = lambda v: (v + 255) // 256 * 256      # noqa: E731
    o0 = al(8 * S); o1 = o0 + al(32 * S * cap); o2 = o1 + al(4 * S * cap); o3 = o2 + al(4 * S * cap)
    assert o3 == len(h) == hip.lib().mscnn_detections_candidates_bytes(S, cap)
    return h[:8 * S].view(np.int32).reshape(S, 2), h[o0:o1], h[o1:o2], h[o2:o3]


def test_a_list_filled_to_exactly_its_capacity_and_to_one_over(hip):
    """2 images x 1 class; image 0's list ends at exactly cand_cap, then at one over: overflow flag, count -1, the number that wanted
    in, nothing stored past the cap (the buffer was poisoned before the reset: every byte outside the stored slots is still 0xFF),
    and image 1, untouched by it, still equals the witness."""
    classes = [2]
    passes = [Pass(0, [64, 10], 2, seed=21), Pass(1, [65, 0], 2, ratios=(1.5, 1.25), view=FLIP, seed=21)]
    want, _ = witness_case(passes, classes)
    full, few = want[0][3], want[1][3]
    assert full > 100 and 0 < few <= 10
    for cap, over in ((full, False), (full - 1, True)):
        cand = hip.Candidates(2, cap)
        cand.buf.fill_(0xFF)
        hip._check(hip.lib().mscnn_detections_candidates_reset(hip._dev(cand.buf), 2, cap, hip._stream()))
        for p in passes:
            p.add_to(cand, classes, hip.NMS_NULL)
        out, pack = cand.merge(raw_pack=True, pack=torch.full((hip.lib().mscnn_detections_multi_pack_bytes(2, 2 * cap),), 0xFF, dtype=torch.uint8,
                                                             device="cuda"))
        counts, boxes, probs, tags = cand_arrays(hip, cand)
        assert counts.tolist() == [[full, int(over)], [few, 0]]
        stored = [min(full, cap), few]
        for arr, item in ((boxes, 32), (probs, 4), (tags, 4)):
            used = np.zeros(len(arr), bool)
            for s in range(2):
                used[item * s * cap:item * (s * cap + stored[s])] = True
            assert np.all(arr[~used] == 0xFF), "a byte outside the stored slots was written"
            assert not np.all(arr[used] == 0xFF)
        table = pack[:48].view(np.int32).reshape(3, 4)
        assert table[0].tolist() == [2, cap, 2 * cap, 0] and table[2].tolist() == [len(want[1][0]), few, cap, 0]
        assert_equals_witness(out[1:], want[1:])
        d0 = pack[48:48 + 40 * 2 * cap].reshape(2 * cap, 40)
        if over:
            assert out[0] == (None, None, full) and table[1].tolist() == [-1, full, 0, 0]
            assert np.all(d0[:cap] == 0xFF), "an overflowed list must not emit rows"
        else:
            assert table[1].tolist() == [len(want[0][0]), full, 0, 0]
            assert_equals_witness(out[:1], want[:1])
            assert np.all(d0[len(want[0][0]):cap] == 0xFF), "rows of a slot past its count are left as they were"
        assert np.all(d0[cap + len(want[1][0]):] == 0xFF)


def dense_pass(k, n, seed):
    """n rows, every one a survivor (no filtered row): clusters of about five boxes on a 16-column grid."""
    rng = np.random.default_rng(seed + k)
    m = rng.integers(0, max(1, n // 5), n)
    xy = np.stack([120 * (m % 16) + 20, 120 * (m // 16) + 20], 1) + rng.integers(-6, 7, (n, 2))
    wh = rng.choice([14, 20, 32, 48], (n, 2))
    p = Pass(k, [0], 2, hw=(20000, 20000), seed=seed)
    p.rows = [n]
    p.props = np.ascontiguousarray(np.concatenate([np.zeros((n, 1)), xy, xy + wh, rng.uniform(-1, 1, (n, 1))], 1).astype(np.float32))
    p.bbox_pred = (rng.standard_normal((n, 8)) * 0.3).astype(np.float32)
    p.cls_pred = (rng.standard_normal((n, 2)) * 2).astype(np.float32)
    p.row0 = np.array([0, n])
    return p


@pytest.mark.parametrize("n0,n1,tiled", [(2016, 2016, False), (2017, 2016, True)])
def test_4032_candidates_take_the_one_pass_path_and_4033_the_tiled_one(hip, n0, n1, tiled):
    passes = [dense_pass(0, n0, 31), dense_pass(1, n1, 31)]
    want, facts = witness_case(passes, [2])
    assert want[0][3] == n0 + n1 and facts[0] and facts[1] and facts[2] == {0, 1}
    cap = n0 + n1
    assert (hip.lib().mscnn_detections_merge_workspace_bytes(1, cap) == hip.lib().mscnn_detections_workspace_bytes(cap)) == tiled
    cand, got = device_case(hip, passes, [2], cap)
    assert_equals_witness(got, want)
    if tiled:      # a non-default type is refused there before any launch: the poisoned pack is untouched
        pack = torch.full((hip.lib().mscnn_detections_multi_pack_bytes(1, cap),), 0xFF, dtype=torch.uint8, device="cuda")
        for nms, text in ((dict(type="max"), "type 1, ovr_dnm 0"), (dict(ovr_dnm="min"), "type 0, ovr_dnm 1")):
            with pytest.raises(hip.MscnnError, match=f"{cap} slots > 4032.*{text}"):
                cand.merge(nms=nms, pack=pack)
        torch.cuda.synchronize()
        assert guarded.all_poison(pack)
    else:
        _, got = device_case(hip, passes, [2], cap, nms=dict(type="max", ovr_dnm="min"))
        assert_equals_witness(got, witness_case(passes, [2], 0.5, "max", "min")[0])


# ---- the plain adds on the list kernel: everything that can meet in one call, the buffer byte for byte ------------------------------------
ROWS17 = [257, 0, 5, 64, 1, 63, 65, 3, 0, 256, 6, 4, 2, 5, 3, 6, 4]      # one step past 256, images without rows, 17 images
VIEWS17 = [FLIP if i % 3 == 1 else (0.0, 0.0, 0) for i in range(17)]      # mirrored images among plain ones


def expected_buffer(hip, S, cap, lists):
    """The bytes of a candidate buffer that was poisoned, reset and given lists[s] = [(rows [n, 5] float64, tags [n])] in add order:
    counts {n, 0}, the slots in order, every other byte still 0xFF."""
    al = lambda v: (v + 255) // 256 * 256      # noqa: E731
    o0 = al(8 * S); o1 = o0 + al(32 * S * cap); o2 = o1 + al(4 * S * cap); o3 = o2 + al(4 * S * cap)
    assert o3 == hip.lib().mscnn_detections_candidates_bytes(S, cap)
    buf = np.full(o3, 0xFF, np.uint8)
    for s, passes in enumerate(lists):
        rows = np.concatenate([r for r, _ in passes])
        tags = np.concatenate([t for _, t in passes]).astype(np.int32)
        n = len(rows)
        assert n <= cap
        buf[8 * s:8 * s + 8] = np.array([n, 0], np.int32).view(np.uint8)
        buf[o0 + 32 * s * cap:o0 + 32 * (s * cap + n)] = np.ascontiguousarray(rows[:, :4]).view(np.uint8).ravel()
        buf[o1 + 4 * s * cap:o1 + 4 * (s * cap + n)] = rows[:, 4].astype(np.float32).view(np.uint8)
        buf[o2 + 4 * s * cap:o2 + 4 * (s * cap + n)] = tags.view(np.uint8)
    return buf


def poisoned_candidates(hip, S, cap):
    cand = hip.Candidates(S, cap)
    cand.buf.fill_(0xFF)
    hip._check(hip.lib().mscnn_detections_candidates_reset(hip._dev(cand.buf), S, cap, hip._stream()))
    return cand


def test_plain_add_of_34_segments_with_views_thr_and_257_rows_fills_the_buffer_like_the_witness(hip):
    """17 images x 2 classes = 34 lists (two launches), images of 257 and of 0 rows, a flip on some images, thr and det_thr set, two
    forwards: every byte of the candidate buffer is the witness's."""
    classes, thr = [2, 3], 0.2
    passes = [Pass(0, ROWS17, 4, ratios=(1.5, 1.25), seed=51), Pass(1, ROWS17[::-1], 4, ratios=(1.0, 0.75), seed=51)]
    passes[0].cls_pred[256] = [0.0, 5.0, 0.0, 0.0]      # (the one row of image 0's second step of 256 is kept for class 2)
    det_thr = float(np.float32(0.25))
    S, cap = 17 * len(classes), 2 * 257
    cand = poisoned_candidates(hip, S, cap)
    lists = [[] for _ in range(S)]
    for k, p in enumerate(passes):
        segs = [p.seg_kw(c) for _ in range(17) for c in classes]
        cand.add(dev(p.bbox_pred), dev(p.cls_pred), dev(p.props), 17, segs, views=VIEWS17, nms=dict(thr=thr, det_thr=det_thr))
        for i in range(17):
            for ci, c in enumerate(classes):
                p.view = VIEWS17[i]
                rows, ids = p.witness_rows(i, c, thr, det_thr)
                lists[i * len(classes) + ci].append((rows, (k << 24) | ids))
    kept = [sum(len(r) for r, _ in l) for l in lists]
    unfiltered = sum(len(p.witness_rows(0, 2)[0]) for p in passes)
    assert 0 < kept[0] < unfiltered and kept[16] == kept[17] == 0 and 256 in (lists[0][0][1] & 0xffffff), \
        "the thresholds, the empty image or the second step show nothing"
    assert np.array_equal(cand.buf.cpu().numpy(), expected_buffer(hip, S, cap, lists))


def test_cascade_add_of_68_segments_with_views_thr_and_257_rows_fills_the_buffer_like_the_witness(hip):
    """The same meeting for _cascade_add: 17 images x 2 outputs x 2 classes = 68 lists (three launches)."""
    classes, O, thr, det_thr = [1, 2], 2, 0.3, 0.1
    specs = [dict(ratios=(1.5, 1.25)), dict(ratios=(1.0, 0.75))]
    fw = [cascade_pass(k, ROWS17, O, 2, seed=53, **sp) for k, sp in enumerate(specs)]
    fw[0][0][1][256] = 0.9                                # (the one row of image 0's second step of 256 is kept)
    K = O * len(classes)
    S, cap = 17 * K, 2 * 257
    cand = poisoned_candidates(hip, S, cap)
    row0 = np.concatenate([[0], np.cumsum(ROWS17)])
    lists = [[] for _ in range(S)]
    for k, sp in enumerate(specs):
        segs = [dict(cls_id=c, ratios=sp["ratios"], org_hw=FRAME, nms_overlap=0.5) for _ in range(17) for _ in range(O) for c in classes]
        cand.cascade_add([tuple(dev(b) for b in o) for o in fw[k]], 17, segs, det_thr=det_thr, views=VIEWS17, nms=dict(thr=thr))
        for s in range(S):
            i, o, c = s // K, (s % K) // len(classes), classes[s % len(classes)]
            boxes, prob, props = fw[k][o]
            sl = slice(row0[i], row0[i + 1])
            r, ids = mw.cascade_rows(boxes[sl], prob[sl], props[sl], c, ratios=sp["ratios"], org_hw=FRAME, det_thr=det_thr, thr=thr)
            lists[s].append((mw.apply_view(r, FRAME[1], VIEWS17[i]), (k << 24) | (ids + row0[i])))
    kept = [sum(len(r) for r, _ in l) for l in lists]
    assert 0 < kept[0] < 2 * 256 and kept[K] == 0 and kept[-1] > 0 and 256 in (lists[0][0][1] & 0xffffff), \
        "the threshold, the empty image or the second step show nothing"
    assert np.array_equal(cand.buf.cpu().numpy(), expected_buffer(hip, S, cap, lists))


# ---- the buffer contract of the three ops ----------------------------------------------------------------------------------------------------
@pytest.fixture
def arena(hip, monkeypatch):
    a = guarded.Arena("cuda")
    monkeypatch.setattr(hip, "torch", guarded.GuardedTorch(torch, a))
    yield a
    torch.cuda.synchronize()
    a.check()


@pytest.mark.parametrize("cap", [200, 4100])
def test_buffer_contract_of_reset_add_and_merge(hip, arena, cap):
    """The candidate buffer, the workspace and the pack between guard bands, the blobs as guarded inputs: guards intact after the
    three ops (both merge paths), the inputs unwritten, pack rows past a count still poison; unaligned bases are refused."""
    classes = [2, 3]
    passes = [Pass(0, [65, 64], 4, seed=41), Pass(1, [63, 66], 4, ratios=(1.5, 1.25), view=FLIP, seed=41)]
    want, _ = witness_case(passes, classes)
    S = 4
    cand = hip.Candidates(S, cap)                         # (its buffer comes from the arena: born poison, reset by the op)
    assert not arena.record(cand.buf).is_input
    for p in passes:
        segs = [p.seg_kw(c) for _ in range(2) for c in classes]
        cand.add(arena.input(p.bbox_pred, np.nan), arena.input(p.cls_pred, np.nan), arena.input(p.props, np.nan), 2, segs,
                 views=None if p.view is None else [p.view] * 2)
    nbytes = hip.lib().mscnn_detections_multi_pack_bytes(S, S * cap)
    pack = arena.alloc(nbytes, torch.uint8)
    ws = arena.alloc(hip.lib().mscnn_detections_merge_workspace_bytes(S, cap), torch.uint8)
    out, h = cand.merge(raw_pack=True, pack=pack, ws=ws)
    torch.cuda.synchronize()
    arena.check()
    assert_equals_witness(out, want)
    dets = h[16 * (S + 1):16 * (S + 1) + 40 * S * cap].reshape(S * cap, 40)
    ids = h[16 * (S + 1) + 40 * S * cap:16 * (S + 1) + 44 * S * cap].reshape(S * cap, 4)
    for s in range(S):
        n = len(want[s][0])
        assert n > 0 and not np.all(dets[s * cap:s * cap + n] == 0xFF)
        assert np.all(dets[s * cap + n:(s + 1) * cap] == 0xFF) and np.all(ids[s * cap + n:(s + 1) * cap] == 0xFF)
    assert np.all(h[16 * (S + 1) + 44 * S * cap:] == 0xFF)
    # unaligned bases: refused, nothing written
    before = cand.buf.clone()
    L = hip.lib()
    off = arena.offset_view(cand.buf, 8)
    p = passes[0]
    descs = (hip.DetectionsDesc * S)()
    for s, kw in enumerate([p.seg_kw(c) for _ in range(2) for c in classes]):
        hip._fill_desc(descs[s], 4, kw)
    blobs = [hip._dev(arena.input(b, np.nan)) for b in (p.bbox_pred, p.cls_pred, p.props)]
    assert L.mscnn_detections_candidates_reset(hip._dev(off), S, cap, hip._stream()) != 0 and "16-byte aligned" in L.mscnn_last_error().decode()
    assert L.mscnn_detections_candidates_add(descs, None, None, 0, 2, 2, *blobs, len(p.props), hip._dev(off), cap, hip._stream()) != 0
    assert "cand must be 16-byte aligned" in L.mscnn_last_error().decode()
    ov = (hip.C.c_double * S)(*([0.5] * S))
    pack2 = arena.alloc(nbytes + 16, torch.uint8)
    ws2 = arena.alloc(ws.numel() + 16, torch.uint8)
    for c_, w_, p_, what in ((off, ws, pack2, "cand"), (cand.buf, ws2[8:], pack2, "workspace"), (cand.buf, ws, pack2[8:], "pack_dev")):
        assert L.mscnn_detections_merge_fwd(ov, None, S, hip._dev(c_), cap, hip._dev(p_), hip._dev(w_), hip.C.c_size_t(ws.numel()), hip._stream()) != 0
        assert f"{what} must be 16-byte aligned" in L.mscnn_last_error().decode()
    torch.cuda.synchronize()
    assert guarded.all_poison(pack2) and guarded.all_poison(ws2) and torch.equal(cand.buf, before)


# ---- Net level ---------------------------------------------------------------------------------------------------------------------------------
def frame_u8(h, w, seed):
    x = synth.frame(h, w, seed=seed, org_hw=(h, w))[0].transpose(1, 2, 0)[:, :, ::-1] + np.array([123.0, 117.0, 104.0])
    return np.ascontiguousarray(np.clip(np.round(x), 0, 255).astype(np.uint8))


def test_net_merge_two_input_sizes_and_a_flip_on_a_plain_net(hip):
    kw = dict(height=192, width=640, max_nms_num=200)
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", **kw))
    synth.load_into(n, "mid")
    img = frame_u8(375, 1242, 41)
    classes = [2, 3]
    forwards = [(192, 640, False), (160, 512, False), (160, 512, True)]
    n.detect_merge_begin(1, len(classes), 3 * 200)
    with pytest.raises(mnet.NetError, match="detect_merge_begin: a merge of 1 images x 2 slots with 0 forwards added is open"):
        n.detect_merge_begin(1, 2, 100)
    lists = {c: [] for c in classes}
    for H, W, flipped in forwards:
        n.reshape_input("data", (1, 3, H, W))
        params = n.set_images("data", [np.ascontiguousarray(img[:, ::-1]) if flipped else img])
        n.forward()
        view = (0.0, 0.0, 1) if flipped else None
        n.detect_merge_add(params, classes, views=None if view is None else [dict(flip_x=1)])
        R = n.blob_shape("proposals_score")[0]
        blobs = [n.get_blob(b).reshape(R, -1) for b in ("bbox_pred", "cls_pred", "proposals_score")]
        for c in classes:
            rows, ids = mw.plain_rows(*blobs, c, bbox_stds=STD, proposal_thr=-10.0, ratios=params[0]["ratios"], org_hw=params[0]["org_hw"])
            lists[c].append((mw.apply_view(rows, params[0]["org_hw"][1], view), ids))
    with pytest.raises(mnet.NetError, match="nms_overlap 0.4, the first forward of this merge was added with 0.5"):
        n.detect_merge_add([dict(params[0], nms_overlap=0.4)], classes)
    per_image, cands = n.detect_merge_end()
    with pytest.raises(mnet.NetError, match="detect_merge_end: no merge is open"):
        n.detect_merge_end()
    total = 0
    for ci, c in enumerate(classes):
        wd, wp, wr, wc = mw.merge(lists[c])
        dets, pas, row = per_image[0][ci]
        assert cands[0][ci] == wc and np.array_equal(pas, wp) and np.array_equal(row, wr) and same_bits(dets, wd), c
        assert len(set(wp.tolist())) >= 2, "the forwards do not interact on this net: the case shows nothing"
        total += len(dets)
    assert total > 3
    # refusals that are decided before anything is enqueued
    R = n.blob_shape("proposals_score")[0]
    n.detect_merge_begin(1, len(classes), R - 1)
    with pytest.raises(mnet.NetError, match=f"0 ROI rows, this one {R}: more than cand_cap {R - 1}"):
        n.detect_merge_add(params, classes)
    with pytest.raises(mnet.NetError, match="no forward has been added"):
        n.detect_merge_end()
    n.detect_merge_begin(2, len(classes), 1000)
    with pytest.raises(mnet.NetError, match="begun with 2 images but the net's input holds 1"):
        n.detect_merge_add(params + params, classes)
    with pytest.raises(mnet.NetError):
        n.detect_merge_end()
    # the merge leaves nothing behind: a whole forward + detect_multi afterwards is a fresh net's, bit for bit
    fresh = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", **kw))
    synth.load_into(fresh, "mid")
    res = []
    for net in (n, fresh):
        net.reshape_input("data", (1, 3, 192, 640))
        p = net.set_images("data", [img])
        net.forward()
        res.append(net.detect_multi(p, classes))
    assert res[0][1] == res[1][1]
    for ci in range(len(classes)):
        assert same_bits(res[0][0][0][ci][0], res[1][0][0][ci][0]) and np.array_equal(res[0][0][0][ci][1], res[1][0][0][ci][1])


def test_net_merge_two_input_sizes_on_a_cascade_net(hip):
    kw = dict(height=192, width=448, max_nms_num=150)
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/cascade-mscnn-7s-576-2x", **kw))
    synth.load_into(n, "mid")
    img = frame_u8(375, 1242, 43)
    classes = [2]
    outputs = [("output_bbox_1st", "cls_prob_1st", "proposals"), ("output_bbox_2nd", "cls_prob_2nd", "proposals_2nd"),
               ("output_bbox_3rd", "cls_prob_3rd_avg" if "cls_prob_3rd_avg" in n.blob_names else "cls_prob_3rd", "proposals_3rd")]
    n.detect_merge_begin(1, len(outputs) * len(classes), 2 * 150)
    lists = [[] for _ in outputs]
    for H, W in ((192, 448), (160, 384)):
        n.reshape_input("data", (1, 3, H, W))
        params = n.set_images("data", [img])
        n.forward()
        n.detect_cascade_merge_add(params, outputs, classes, det_thr=0.05)
        for o, (bb, pb, qb) in enumerate(outputs):
            R = n.blob_shape(bb)[0]
            rows, ids = mw.cascade_rows(n.get_blob(bb).reshape(R, 5), n.get_blob(pb).reshape(R, -1), n.get_blob(qb).reshape(R, 5), 2,
                                        ratios=params[0]["ratios"], org_hw=params[0]["org_hw"], det_thr=0.05)
            lists[o].append((rows, ids))
    per_image, cands = n.detect_merge_end()
    total = 0
    for o in range(len(outputs)):
        wd, wp, wr, wc = mw.merge(lists[o])
        dets, pas, row = per_image[0][o]
        assert cands[0][o] == wc and np.array_equal(pas, wp) and np.array_equal(row, wr) and same_bits(dets, wd), o
        total += len(dets)
    assert total > 3
    fresh = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/cascade-mscnn-7s-576-2x", **kw))
    synth.load_into(fresh, "mid")
    res = []
    for net in (n, fresh):
        net.reshape_input("data", (1, 3, 192, 448))
        p = net.set_images("data", [img])
        net.forward()
        res.append(net.detect_cascade_multi(p, outputs, classes))
    assert res[0][1] == res[1][1]
    for o in range(len(outputs)):
        assert same_bits(res[0][0][0][o][0][0], res[1][0][0][o][0][0]) and np.array_equal(res[0][0][0][o][0][1], res[1][0][0][o][0][1])
