"""Box voting behind the merge on the GPU: mscnn_detections_merge_vote_fwd through the HIP ABI on synthetic, seeded candidate lists
(both merge paths, the plain and the cascade stage) and Net.set_box_voting on a reduced deploy.  The pack after the vote is compared
BYTE FOR BYTE with the pack before it in which the numpy witness (tests/vote_witness.py: the op's documented summation order) has
replaced the four box doubles of every kept row -- so one comparison shows the voted boxes and that nothing else was written.  No
tolerance is involved; no pin on the reference, whose scripts neither merge nor vote.

Each witness case first shows ON THE WITNESS'S OWN RESULT that some kept row has voters from more than one pass, a voter scored above
itself (a candidate another kept box suppressed) and fewer than two voters: a case can not pass with a vote that does nothing.

The shapes are the smallest at which the kernel can go wrong: lists of 1, 2, 63, 64, 65, 129 and 200 candidates (one under, on and
over a wave's 64 lanes, over two rounds of them, a full list of 200 slots under the 256-slot tile), an empty and an overflowed list,
2000 kept rows (more groups of four than the grid has workgroups), and 4033 slots (the tiled merge, 16 tiles of candidates)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import guarded                                   # noqa: E402
import merge_witness as mw                       # noqa: E402
import vote_witness as vw                        # noqa: E402
from mscnn_amd import net as mnet, synth, zoo   # noqa: E402

STD = (0.1, 0.1, 0.2, 0.2)
FRAME = (1800, 1600)                     # (H, W) of the original image every synthetic case lives in
FLIP = (0.0, 0.0, 1)
CAP = 200
NET_CAP = 2 * 2000                       # the Net-level case: two forwards x the deploy's max_nms_num


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


# ---- synthetic passes: every row is a candidate ------------------------------------------------------------------------------------------------
def boxes_in_frame(n, k, rng, clusters=6):
    """n boxes [x y w h] in frame coordinates: members of 6 clusters every pass and image shares (boxes of different passes overlap),
    row 0 alone at a place of the pass's own (a kept row whose only voter is itself)."""
    m = rng.integers(0, clusters, n)
    x = 100 + 300 * (m % 3) + rng.integers(-5, 6, n)
    y = 100 + 300 * (m // 3) + rng.integers(-5, 6, n)
    w = rng.choice([28, 32, 36], n)
    h = rng.choice([28, 32, 36], n)
    if n:
        x[0], y[0], w[0], h[0] = 100 + 150 * k, 1500, 20, 20
    return x.astype(np.float64), y.astype(np.float64), w.astype(np.float64), h.astype(np.float64)


def into_view(x, w, view, view_w):
    return x if view is None else view_w - (x + w)      # (the views of this file: the identity and the mirror)


class PlainPass:
    """One forward of the plain stage: rows per image, its ratios and view; no row is filtered, so a list's length is the rows added."""

    def __init__(self, k, rows, ratios=(1.0, 1.0), view=None, seed=0, clusters=6):
        rng = np.random.default_rng(1000 * seed + k)
        self.k, self.rows, self.ratios, self.view = k, rows, ratios, view
        parts = []
        for i, n in enumerate(rows):
            x, y, w, h = boxes_in_frame(n, k, rng, clusters)
            xv = into_view(x, w, view, FRAME[1])
            parts.append(np.stack([np.full(n, float(i)), xv * ratios[1], y * ratios[0], (xv + w) * ratios[1], (y + h) * ratios[0],
                                   rng.uniform(-1, 1, n)], 1).astype(np.float32))
        self.props = np.ascontiguousarray(np.concatenate(parts))
        R = len(self.props)
        self.bbox_pred = (rng.standard_normal((R, 8)) * 0.3).astype(np.float32)
        self.cls_pred = (rng.standard_normal((R, 2)) * 2).astype(np.float32)
        self.row0 = np.concatenate([[0], np.cumsum(rows)]).astype(int)

    def seg_kw(self):
        return dict(cls_id=2, bbox_mean=(0, 0, 0, 0), bbox_std=STD, proposal_thr=-10.0, ratios=self.ratios, org_hw=FRAME, nms_overlap=0.5)

    def witness_rows(self, i):
        sl = slice(self.row0[i], self.row0[i + 1])
        rows, ids = mw.plain_rows(self.bbox_pred[sl], self.cls_pred[sl], self.props[sl], 2, bbox_stds=STD, proposal_thr=-10.0,
                                  ratios=self.ratios, org_hw=FRAME)
        return mw.apply_view(rows, FRAME[1], self.view), ids + self.row0[i]

    def add_to(self, cand, arena=None):
        B = len(self.rows)
        up = dev if arena is None else (lambda b: arena.input(b, np.nan))
        cand.add(up(self.bbox_pred), up(self.cls_pred), up(self.props), B, [self.seg_kw()] * B, views=None if self.view is None else [self.view] * B)


class CascadePass:
    """One forward of the cascade stage, one output: the decoded boxes are the cluster boxes in the view's net coordinates
    ([x1 y1 x2 y2], x2 = x1 + w - 1: the rows come out w wide at ratio 1 under the stage's + 1)."""

    def __init__(self, k, rows, ratios=(1.0, 1.0), view=None, seed=0):
        rng = np.random.default_rng(5000 * seed + k)
        self.k, self.rows, self.ratios, self.view = k, rows, ratios, view
        parts = []
        for i, n in enumerate(rows):
            x, y, w, h = boxes_in_frame(n, k, rng)
            xv = into_view(x, w, view, FRAME[1])
            parts.append(np.stack([np.full(n, float(i)), xv * ratios[1], y * ratios[0], (xv + w - 1) * ratios[1], (y + h - 1) * ratios[0]], 1))
        self.boxes = np.ascontiguousarray(np.concatenate(parts).astype(np.float32))
        self.prob = rng.uniform(0.02, 0.98, (len(self.boxes), 2)).astype(np.float32)
        self.row0 = np.concatenate([[0], np.cumsum(rows)]).astype(int)

    def seg_kw(self):
        return dict(cls_id=2, ratios=self.ratios, org_hw=FRAME, nms_overlap=0.5)

    def witness_rows(self, i):
        sl = slice(self.row0[i], self.row0[i + 1])
        rows, ids = mw.cascade_rows(self.boxes[sl], self.prob[sl], self.boxes[sl], 2, ratios=self.ratios, org_hw=FRAME)
        return mw.apply_view(rows, FRAME[1], self.view), ids + self.row0[i]

    def add_to(self, cand, arena=None):
        B = len(self.rows)
        cand.cascade_add([(dev(self.boxes), dev(self.prob), dev(self.boxes))], B, [self.seg_kw()] * B, views=None if self.view is None else [self.view] * B)


# ---- the expectation: the un-voted pack with the witness's boxes in its kept rows -----------------------------------------------------------
def pack_views(h, S, cap):
    table = 16 * (S + 1)
    return (h[:table].view(np.int32).reshape(S + 1, 4), h[table:table + 40 * S * cap].view(np.float64).reshape(S * cap, 5),
            h[table + 40 * S * cap:table + 44 * S * cap].view(np.int32))


def expected_pack(h0, passes, B, cap, thr):
    """(the bytes the pack must hold after the vote, the facts over all segments, kept rows, rows the vote moved).  Also checks the
    un-voted pack h0 against merge_witness: the vote starts from the right rows."""
    want = h0.copy()
    hdr, dets, tags = pack_views(want, B, cap)
    facts = np.zeros(3, bool)
    kept = moved = 0
    for s in range(B):
        lists = [p.witness_rows(s) for p in passes]
        n = sum(len(r) for r, _ in lists)
        assert hdr[1 + s, 1] == n, (s, hdr[1 + s].tolist(), n)
        if n > cap:
            assert hdr[1 + s, 0] == -1, "an overflowed list"
            continue
        d, voted, pas, row, _, who, cand_pass = vw.vote_segment(lists, thr)
        D = len(d)
        assert hdr[1 + s, 0] == D and same_bits(dets[s * cap:s * cap + D], d), (s, "the un-voted pack is not the merge witness's")
        assert np.array_equal(tags[s * cap:s * cap + D], (pas.astype(np.int32) << 24) | row), s
        if D:
            facts |= np.array(vw.vote_facts(d, vw.candidates_of(lists)[0], cand_pass, who))
        for k in range(D):
            if len(who[k]) < 2:
                assert same_bits(voted[k], d[k]), "fewer than two voters: the witness leaves the row bit for bit"
        dets[s * cap:s * cap + D] = voted
        kept += D
        moved += int(np.count_nonzero(np.any(voted[:, :4] != d[:, :4], 1)))
    return want, tuple(bool(f) for f in facts), kept, moved


def merge_then_vote(hip, cand, thr, pack=None):
    """(pack bytes after the merge, pack bytes after the vote on that very pack)."""
    S, cap = cand.S, cand.cap
    if pack is None:
        pack = torch.full((hip.lib().mscnn_detections_multi_pack_bytes(S, S * cap),), 0xFF, dtype=torch.uint8, device="cuda")
    _, h0 = cand.merge(raw_pack=True, pack=pack)                    # (poisoned past each count: "rows of a slot past its count")
    cand.vote(pack, thr)
    torch.cuda.synchronize()
    return h0, pack.cpu().numpy()


# list lengths of images 0 and 3 as (pass 0, pass 1) rows; image 1 has no rows at all, image 2 overflows its 200 slots
LISTS = {"1_and_129": ((1, 0), (64, 65)), "2_and_200": ((1, 1), (100, 100)), "63_and_65": ((30, 33), (33, 32)), "64_and_129": ((32, 32), (65, 64))}


@pytest.mark.parametrize("thr", [0.5, 0.3])
@pytest.mark.parametrize("stage", ["plain", "cascade"])
@pytest.mark.parametrize("name", list(LISTS))
def test_vote_is_bit_equal_to_the_witness(hip, name, stage, thr):
    (a0, a1), (c0, c1) = LISTS[name]
    P = PlainPass if stage == "plain" else CascadePass
    passes = [P(0, [a0, 0, 150, c0], ratios=(1.0, 1.0), seed=5), P(1, [a1, 0, 150, c1], ratios=(1.5, 1.25), view=FLIP, seed=5)]
    cand = hip.Candidates(4, CAP)
    for p in passes:
        p.add_to(cand)
    assert [c[0] for c in cand.counts()] == [a0 + a1, 0, 300, c0 + c1] and [c[1] for c in cand.counts()] == [0, 0, 1, 0]
    h0, h1 = merge_then_vote(hip, cand, thr)
    want, (multi, higher, lonely), kept, moved = expected_pack(h0, passes, 4, CAP, thr)
    assert multi, "no kept row has voters from more than one pass: the case shows nothing"
    assert higher, "no kept row has a voter scored above itself: the case shows nothing"
    assert lonely, "no kept row has fewer than two voters: the case shows nothing"
    assert kept >= 8 and moved >= 3 and not np.array_equal(h0, want)
    assert np.array_equal(h1, want), np.flatnonzero(h1 != want)[:8]
    hdr = pack_views(h1, 4, CAP)[0]
    assert hdr[0].tolist() == [4, CAP, 4 * CAP, 0] and hdr[2].tolist() == [0, 0, CAP, 0] and hdr[3].tolist() == [-1, 300, 2 * CAP, 0]


def test_more_voters_than_a_wave_has_lanes(hip):
    """One cluster and a threshold low enough that a kept row of the full 200-slot list has more than 64 voters: some partial sum adds several voters
    in ascending slot order before the butterfly."""
    passes = [PlainPass(0, [1, 0, 150, 100], seed=5, clusters=1), PlainPass(1, [1, 0, 150, 100], ratios=(1.5, 1.25), view=FLIP, seed=5, clusters=1)]
    d, voted, _, _, _, who, _ = vw.vote_segment([p.witness_rows(3) for p in passes], 0.05)
    assert max(len(w) for w in who) > 64, max(len(w) for w in who)
    cand = hip.Candidates(4, CAP)
    for p in passes:
        p.add_to(cand)
    h0, h1 = merge_then_vote(hip, cand, 0.05)
    want, facts, kept, moved = expected_pack(h0, passes, 4, CAP, 0.05)
    assert moved >= 3 and np.array_equal(h1, want), np.flatnonzero(h1 != want)[:8]


def test_the_vote_is_not_idempotent_and_a_second_vote_is_the_witness_on_the_moved_boxes(hip):
    passes = [PlainPass(0, [1, 0, 150, 64], seed=5), PlainPass(1, [0, 0, 150, 65], ratios=(1.5, 1.25), view=FLIP, seed=5)]
    cand = hip.Candidates(4, CAP)
    for p in passes:
        p.add_to(cand)
    h0, h1 = merge_then_vote(hip, cand, 0.5)
    pack = dev(h1)
    cand.vote(pack, 0.5)
    h2 = pack.cpu().numpy()
    assert not np.array_equal(h2, h1), "a second vote runs around the moved boxes (documented: not idempotent)"
    # the second vote is the witness's on the pack the first one left
    hdr, d1, _ = pack_views(h1.copy(), 4, CAP)
    want = h1.copy()
    _, dw, _ = pack_views(want, 4, CAP)
    D = int(hdr[4, 0])
    dw[3 * CAP:3 * CAP + D] = vw.vote(d1[3 * CAP:3 * CAP + D], vw.candidates_of([p.witness_rows(3) for p in passes])[0], 0.5)[0]
    assert np.array_equal(h2, want)


# ---- more kept rows than one pass of the grid ---------------------------------------------------------------------------------------------------
def grid_blobs(n, shift=0, logit=None):
    """n disjoint 20 x 20 boxes on a 50-column grid (40 pixels apart) as plain-stage blobs with zero regression at ratio 1: the rows
    come out as the integer boxes they are.  shift: all of them that many pixels to the right."""
    i = np.arange(n)
    x, y = 10.0 + 40 * (i % 50) + shift, 10.0 + 40 * (i // 50)
    props = np.stack([np.zeros(n), x, y, x + 20, y + 20, np.zeros(n)], 1).astype(np.float32)
    cls_pred = np.zeros((n, 2), np.float32)
    cls_pred[:, 1] = np.linspace(-2, 2, n) if logit is None else logit
    return np.zeros((n, 8), np.float32), cls_pred, props


def test_2000_kept_rows_go_round_the_grid_alone_and_with_a_twin_each(hip):
    n = 2000
    kw = dict(cls_id=2, bbox_mean=(0, 0, 0, 0), bbox_std=STD, proposal_thr=-10.0, ratios=(1.0, 1.0), org_hw=(2000, 2100), nms_overlap=0.5)
    base = grid_blobs(n)
    # disjoint boxes: every row is kept, every row is its own only voter, nothing changes
    cand = hip.Candidates(1, n)
    cand.add(*[dev(b) for b in base], 1, [kw])
    h0, h1 = merge_then_vote(hip, cand, 0.5)
    hdr, dets, _ = pack_views(h1, 1, n)
    assert hdr[1].tolist() == [n, n, 0, 0] and np.array_equal(h0, h1)
    rows, ids = mw.plain_rows(*base, 2, bbox_stds=STD, org_hw=(2000, 2100))
    assert len(rows) == n and same_bits(dets, mw.merge([(rows, ids)])[0])
    # a twin of every box, one pixel to the right and scored lower, from a second forward: 2000 kept rows, two voters each
    twin = grid_blobs(n, shift=1, logit=np.linspace(-2, 2, n) - 0.5)
    cand = hip.Candidates(1, 2 * n)
    cand.add(*[dev(b) for b in base], 1, [kw])
    cand.add(*[dev(b) for b in twin], 1, [kw])
    h0, h1 = merge_then_vote(hip, cand, 0.5)
    lists = [(rows, ids), mw.plain_rows(*twin, 2, bbox_stds=STD, org_hw=(2000, 2100))]
    d, voted, pas, row, cands, who, _ = vw.vote_segment(lists, 0.5)
    assert len(d) == n and cands == 2 * n and all(len(w) == 2 for w in who) and set(pas.tolist()) == {0}
    assert np.all(voted[:, 0] > d[:, 0]) and np.all(voted[:, 0] < d[:, 0] + 1) and np.array_equal(voted[:, 4], d[:, 4])
    want = h0.copy()
    hdr, dw, _ = pack_views(want, 1, 2 * n)
    assert hdr[1].tolist() == [n, 2 * n, 0, 0] and same_bits(dw[:n], d)
    dw[:n] = voted
    assert np.array_equal(h1, want), np.flatnonzero(h1 != want)[:8]


# ---- behind the tiled merge --------------------------------------------------------------------------------------------------------------------
def dense_pass(k, n, seed):
    """n rows, every one a survivor: clusters of about five boxes on a 16-column grid (the construction of the merge's own 4033-slot
    case, rebuilt here)."""
    rng = np.random.default_rng(seed + k)
    m = rng.integers(0, max(1, n // 5), n)
    xy = np.stack([120 * (m % 16) + 20, 120 * (m // 16) + 20], 1) + rng.integers(-6, 7, (n, 2))
    wh = rng.choice([14, 20, 32, 48], (n, 2))
    p = PlainPass(k, [1], seed=seed)
    p.rows = [n]
    p.props = np.ascontiguousarray(np.concatenate([np.zeros((n, 1)), xy, xy + wh, rng.uniform(-1, 1, (n, 1))], 1).astype(np.float32))
    p.bbox_pred = (rng.standard_normal((n, 8)) * 0.3).astype(np.float32)
    p.cls_pred = (rng.standard_normal((n, 2)) * 2).astype(np.float32)
    p.row0 = np.array([0, n])
    p.seg_kw = lambda: dict(cls_id=2, bbox_mean=(0, 0, 0, 0), bbox_std=STD, proposal_thr=-10.0, ratios=(1.0, 1.0), org_hw=(20000, 20000), nms_overlap=0.5)
    p.witness_rows = lambda i: mw.plain_rows(p.bbox_pred, p.cls_pred, p.props, 2, bbox_stds=STD, proposal_thr=-10.0, org_hw=(20000, 20000))
    return p


def test_vote_behind_the_tiled_merge_of_4033_slots(hip):
    passes = [dense_pass(0, 2017, 31), dense_pass(1, 2016, 31)]
    cap = 4033
    assert hip.lib().mscnn_detections_merge_workspace_bytes(1, cap) == hip.lib().mscnn_detections_workspace_bytes(cap), "the tiled path"
    cand = hip.Candidates(1, cap)
    for p in passes:
        p.add_to(cand)
    h0, h1 = merge_then_vote(hip, cand, 0.5)
    want, (multi, higher, lonely), kept, moved = expected_pack(h0, passes, 1, cap, 0.5)
    assert multi and higher and lonely and kept > 500 and moved > 100
    assert np.array_equal(h1, want), np.flatnonzero(h1 != want)[:8]


# ---- the buffer contract ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def arena(hip, monkeypatch):
    a = guarded.Arena("cuda")
    monkeypatch.setattr(hip, "torch", guarded.GuardedTorch(torch, a))
    yield a
    torch.cuda.synchronize()
    a.check()


def test_buffer_contract_of_the_vote(hip, arena):
    """The candidate buffer and the pack between guard bands, the pack poisoned past each count: after the vote the guards are intact,
    the candidate buffer is unwritten, and of the pack only the four box doubles of voted rows differ -- prob column, tags, header,
    table, rows past a count and every slot of the overflowed segment as they were.  An unaligned base is refused, nothing written."""
    passes = [PlainPass(0, [30, 0, 150, 64], seed=5), PlainPass(1, [33, 0, 150, 65], ratios=(1.5, 1.25), view=FLIP, seed=5)]
    S = 4
    cand = hip.Candidates(S, CAP)                          # (its buffer comes from the arena: born poison, reset by the op)
    assert not arena.record(cand.buf).is_input
    for p in passes:
        p.add_to(cand, arena)
    nbytes = hip.lib().mscnn_detections_multi_pack_bytes(S, S * CAP)
    pack = arena.alloc(nbytes, torch.uint8)
    _, h0 = cand.merge(raw_pack=True, pack=pack)
    before = cand.buf.clone()
    cand.vote(pack, 0.5)
    torch.cuda.synchronize()
    arena.check()
    assert torch.equal(cand.buf, before), "the vote wrote the candidate buffer"
    h1 = pack.cpu().numpy()
    want, facts, kept, moved = expected_pack(h0, passes, S, CAP, 0.5)
    assert all(facts) and moved >= 3
    assert np.array_equal(h1, want)
    hdr, d0, t0 = pack_views(h0, S, CAP)
    _, d1, t1 = pack_views(h1, S, CAP)
    changed = np.any(d0.view(np.uint64) != d1.view(np.uint64), 1)
    assert np.count_nonzero(changed) == moved
    assert np.array_equal(h0[:16 * (S + 1)], h1[:16 * (S + 1)]) and np.array_equal(t0, t1)                    # header, table, tags
    assert np.array_equal(d0[:, 4].view(np.uint64), d1[:, 4].view(np.uint64))                                  # the prob column
    raw = h1[16 * (S + 1):16 * (S + 1) + 40 * S * CAP].reshape(S * CAP, 40)
    for s in range(S):
        D = max(int(hdr[1 + s, 0]), 0)
        assert not np.any(changed[s * CAP + D:(s + 1) * CAP]) and np.all(raw[s * CAP + D:(s + 1) * CAP] == 0xFF), s
    assert hdr[3, 0] == -1 and np.all(raw[2 * CAP:3 * CAP] == 0xFF), "the overflowed segment's slots"
    assert np.array_equal(h0[16 * (S + 1) + 44 * S * CAP:], h1[16 * (S + 1) + 44 * S * CAP:])
    # unaligned bases: refused, nothing written
    L = hip.lib()
    vp = hip.C.byref(hip.VoteParams(0.5))
    off = arena.offset_view(cand.buf, 8)
    pack2 = arena.alloc(nbytes + 16, torch.uint8)
    for c_, p_, what in ((off, pack2, "cand"), (cand.buf, pack2[8:], "pack_dev")):
        assert L.mscnn_detections_merge_vote_fwd(vp, S, hip._dev(c_), CAP, hip._dev(p_), hip._stream()) != 0
        assert f"detections_merge_vote: {what} must be 16-byte aligned" in L.mscnn_last_error().decode()
    with pytest.raises(hip.MscnnError, match=r"thr 1 is outside \(0, 1\)"):
        cand.vote(pack2, 1.0)
    torch.cuda.synchronize()
    assert guarded.all_poison(pack2) and torch.equal(cand.buf, before) and np.array_equal(pack.cpu().numpy(), h1)


# ---- Net level ----------------------------------------------------------------------------------------------------------------------------------
def frame_u8(h, w, seed):
    x = synth.frame(h, w, seed=seed, org_hw=(h, w))[0].transpose(1, 2, 0)[:, :, ::-1] + np.array([123.0, 117.0, 104.0])
    return np.ascontiguousarray(np.clip(np.round(x), 0, 255).astype(np.uint8))


def test_net_box_voting_is_the_op_behind_the_merge_and_off_again_the_merge_alone(hip):
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=96, width=320))
    synth.load_into(n, "mid")
    img = frame_u8(375, 1242, 41)
    classes = [2, 3]

    def run(keep_blobs):
        """A frame and its mirror, merged: (detect_merge_end's result, the forwards' blobs and params)."""
        fw = []
        n.detect_merge_begin(1, len(classes), NET_CAP)
        for flipped in (False, True):
            params = n.set_images("data", [np.ascontiguousarray(img[:, ::-1]) if flipped else img])
            n.forward()
            n.detect_merge_add(params, classes, views=[dict(flip_x=1)] if flipped else None)
            if keep_blobs:
                R = n.blob_shape("proposals_score")[0]
                fw.append(([n.get_blob(b).reshape(R, -1) for b in ("bbox_pred", "cls_pred", "proposals_score")], params[0], flipped))
        return n.detect_merge_end(), fw

    assert n.get_box_voting() is None
    n.set_box_voting(0.5)
    (voted, cands), fw = run(True)
    n.set_box_voting(None)
    (plain, cands2), _ = run(False)
    assert cands == cands2
    # the same blobs through the ops: Candidates.merge, and merge + vote
    cand = hip.Candidates(len(classes), NET_CAP)
    for blobs, p, flipped in fw:
        segs = [dict(cls_id=c, bbox_mean=(0, 0, 0, 0), bbox_std=STD, proposal_thr=-10.0, ratios=p["ratios"], org_hw=p["org_hw"], nms_overlap=0.5)
                for c in classes]
        cand.add(*[dev(b) for b in blobs], 1, segs, views=[FLIP] if flipped else None)
    ref_plain = cand.merge()
    ref_voted = cand.merge(vote_thr=0.5)
    moved = 0
    for ci in range(len(classes)):
        for got, ref in ((plain, ref_plain), (voted, ref_voted)):
            dets, pas, row = got[0][ci]
            assert same_bits(dets, ref[ci][0]) and np.array_equal((pas << 24) | row, ref[ci][1]) and cands[0][ci] == ref[ci][2], ci
        assert len(voted[0][ci][0]) == len(plain[0][ci][0]) and np.array_equal(voted[0][ci][0][:, 4], plain[0][ci][0][:, 4])
        moved += int(np.count_nonzero(np.any(voted[0][ci][0][:, :4] != plain[0][ci][0][:, :4], 1)))
    assert moved >= 1, "the vote moved no box on this net: the case shows nothing"
