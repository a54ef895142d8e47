"""Soft-NMS over the merged candidates on the GPU: mscnn_detections_merge_soft_fwd through the HIP ABI on synthetic, seeded candidate
lists, and Net.set_soft_nms on a reduced deploy.  No pin on the reference, whose scripts neither merge nor decay a score: the check is
tests/soft_witness.py.

LINEAR is IEEE operations only: the whole pack -- header, table, rows, tags, and every byte the op must leave alone (the pack starts
as 0xFF poison) -- is compared BYTE FOR BYTE with the pack the witness describes.  GAUSSIAN calls exp (OCML's on the device, numpy's
in the witness): boxes, tags and counts are exact, the scores lie within 4 D 2^-52 relative, D = the list's pick count.  Derivation:
the overlap r is bit-identical on both sides (the same IEEE operations on the same boxes); per decay two exp results of at most 1 ulp
each (the documented bound of both libraries) and two roundings of the product differ by at most 3 ulp = 3 * 2^-52 relative, and a
score goes through at most D decays.  The test asserts the condition under which a last-bit difference can not turn a pick: the
witness's min_gap > 1e-9.  The largest difference seen is printed in ulps (profiles/detect_merge_soft.txt records it).

Each witness case first shows ON THE WITNESS'S OWN RESULT that some score was decayed, some candidate was dropped and the pick
order is not the plain score order: a case can not pass with a hard NMS or with a sort.

Shapes, the smallest at which the kernel can go wrong: lists of about 130 candidates (two of a thread's wave rounds), an empty and an
overflowed list, 33 segments (over the 32 of a launch), 4096 and 4097 candidates (the last list in registers, the first one streamed
through the workspace), max_out 1, 7 and 0."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import guarded                                   # noqa: E402
import merge_witness as mw                       # noqa: E402
import soft_witness as sw                        # noqa: E402
import vote_witness as vw                        # noqa: E402
from mscnn_amd import net as mnet, synth, zoo   # noqa: E402

STD = (0.1, 0.1, 0.2, 0.2)
FRAME = (1800, 1600)                     # (H, W) of the original image the clustered cases live in
BIG = (20000, 20000)                     # ... and the dense ones
FLIP = (0.0, 0.0, 1)
OVERLAP = 0.3
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


# ---- synthetic passes: every row is a candidate -----------------------------------------------------------------------------------------------
def clustered(n, rng):
    """n boxes [x y w h]: members of 6 clusters every pass and image shares, a few pixels apart -- most pairs of a cluster overlap
    by more than 0.3, many by more than 0.5."""
    m = rng.integers(0, 6, n)
    return np.stack([100 + 300 * (m % 3) + rng.integers(-5, 6, n), 100 + 300 * (m // 3) + rng.integers(-5, 6, n),
                     rng.choice([28, 32, 36], n), rng.choice([28, 32, 36], n)], 1).astype(np.float64)


def dense(n, rng):
    """n boxes in clusters of about five on a 16-column grid (the construction of the merge's own 4033-slot case)."""
    m = rng.integers(0, max(1, n // 5), n)
    xy = np.stack([120 * (m % 16) + 20, 120 * (m // 16) + 20], 1) + rng.integers(-6, 7, (n, 2))
    return np.concatenate([xy, rng.choice([14, 20, 32, 48], (n, 2))], 1).astype(np.float64)


class Pass:
    """One forward of the plain stage: rows per image, the ratios of its input size and its view (the identity or the mirror); no
    row is filtered, so a list's length is the rows added."""

    def __init__(self, k, rows, ncls=3, ratios=(1.0, 1.0), view=None, hw=FRAME, seed=0, boxes=clustered):
        rng = np.random.default_rng(1000 * seed + k)
        self.k, self.rows, self.ratios, self.view, self.hw, self.ncls = k, rows, ratios, view, hw, ncls
        parts = []
        for i, n in enumerate(rows):
            b = boxes(n, rng)
            x = b[:, 0] if view is None else hw[1] - (b[:, 0] + b[:, 2])
            parts.append(np.stack([np.full(n, float(i)), x * ratios[1], b[:, 1] * ratios[0], (x + b[:, 2]) * ratios[1], (b[:, 1] + b[:, 3]) * ratios[0],
                                   rng.uniform(-1, 1, n)], 1).astype(np.float32))
        self.props = np.ascontiguousarray(np.concatenate(parts))
        R = len(self.props)
        self.bbox_pred = (rng.standard_normal((R, 4 * ncls)) * 0.3).astype(np.float32)
        self.cls_pred = (rng.standard_normal((R, ncls)) * 2).astype(np.float32)
        self.row0 = np.concatenate([[0], np.cumsum(rows)]).astype(int)

    def seg_kw(self, cls_id):
        return dict(cls_id=cls_id, bbox_mean=(0, 0, 0, 0), bbox_std=STD, proposal_thr=-10.0, ratios=self.ratios, org_hw=self.hw, nms_overlap=OVERLAP)

    def witness_rows(self, i, cls_id):
        sl = slice(self.row0[i], self.row0[i + 1])
        rows, ids = mw.plain_rows(self.bbox_pred[sl], self.cls_pred[sl], self.props[sl], cls_id, bbox_stds=STD, proposal_thr=-10.0,
                                  ratios=self.ratios, org_hw=self.hw)
        return mw.apply_view(rows, self.hw[1], self.view), ids + self.row0[i]

    def add_to(self, cand, classes, arena=None):
        B = len(self.rows)
        up = dev if arena is None else (lambda b: arena.input(b, np.nan))
        cand.add(up(self.bbox_pred), up(self.cls_pred), up(self.props), B, [self.seg_kw(c) for _ in range(B) for c in classes],
                 views=None if self.view is None else [self.view] * B)


def lists_of(passes, classes):
    """Per segment (image-major, then class): the passes' (rows, ids) in add order -- soft_witness.soft_segment's argument."""
    return [[p.witness_rows(i, c) for p in passes] for i in range(len(passes[0].rows)) for c in classes]


def filled(hip, passes, classes, cap, arena=None):
    cand = hip.Candidates(len(passes[0].rows) * len(classes), cap)
    for p in passes:
        p.add_to(cand, classes, arena)
    return cand


# ---- the expectation: the poisoned pack with what the witness says the op writes ------------------------------------------------------------
def pack_views(h, S, cap):
    table = 16 * (S + 1)
    return (h[:table].view(np.int32).reshape(S + 1, 4), h[table:table + 40 * S * cap].view(np.float64).reshape(S * cap, 5),
            h[table + 40 * S * cap:table + 44 * S * cap].view(np.int32))


def expected_pack(nbytes, lists, cap, method, **kw):
    """(the bytes a 0xFF-poisoned pack must hold after the op, the witness's result per segment (None: the list overflowed))."""
    S = len(lists)
    want = np.full(nbytes, 0xFF, np.uint8)
    hdr, dets, tags = pack_views(want, S, cap)
    hdr[0] = [S, cap, S * cap, 0]
    res = []
    for s, passes in enumerate(lists):
        n = sum(len(r) for r, _ in passes)
        if n > cap:
            hdr[1 + s] = [-1, n, s * cap, 0]
            res.append(None)
            continue
        d, pas, row, cands, slots, decays, gap = sw.soft_segment(passes, sw.METHODS[method], overlap=OVERLAP, **kw)
        hdr[1 + s] = [len(d), n, s * cap, 0]
        dets[s * cap:s * cap + len(d)] = d
        tags[s * cap:s * cap + len(d)] = (pas.astype(np.int32) << 24) | row
        res.append((d, slots, decays, gap, sw.candidates_of(passes)[0]))
    return want, res


def facts_of(res):
    """soft_witness.soft_facts over all segments of a case."""
    f = np.zeros(3, bool)
    for r in res:
        if r is not None and len(r[4]):
            f |= np.array(sw.soft_facts(r[4], r[0], r[1], r[2]))
    return tuple(bool(v) for v in f)


def run_soft(hip, cand, method, pack=None, ws=None, **kw):
    """The op on a 0xFF-poisoned pack: (merge_soft's result, the pack's bytes)."""
    if pack is None:
        pack = torch.full((hip.lib().mscnn_detections_multi_pack_bytes(cand.S, cand.S * cand.cap),), 0xFF, dtype=torch.uint8, device="cuda")
    out, h = cand.merge_soft(method, raw_pack=True, pack=pack, ws=ws, **kw)
    return out, h


def ulps(a, b):
    """|a - b| in units of the last place of b, elementwise (finite, same sign)."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.abs(a - b) / np.spacing(np.abs(b))


CASES = {
    # 2 passes x 2 images x 2 classes of about 65 rows: a plain view and a flipped, rescaled one
    "S4_two_passes": ([2, 3], lambda: [Pass(0, [65, 64], seed=3), Pass(1, [63, 66], ratios=(1.5, 1.25), view=FLIP, seed=3)]),
    # 11 images x 3 classes = 33 segments: one over a launch's 32; image 4 has no rows at all (count 0)
    "S33_across_the_launch_boundary": ([1, 2, 3], lambda: [Pass(0, [9, 7, 12, 8, 0, 9, 12, 7, 8, 9, 12], seed=5),
                                                           Pass(1, [8, 12, 7, 9, 0, 10, 8, 9, 12, 7, 9], ratios=(1.5, 1.25), view=FLIP, seed=5)]),
}
_cache = {}


def case(name):
    """(classes, passes, lists): built once per module -- the witness rows go through C's expf one by one."""
    if name not in _cache:
        classes, make = CASES[name]
        passes = make()
        _cache[name] = (classes, passes, lists_of(passes, classes))
    return _cache[name]


@pytest.mark.parametrize("max_out,score_thr", [(0, 0.05), (1, 0.05), (7, 0.05), (0, 0.3)])
@pytest.mark.parametrize("name", list(CASES))
def test_linear_is_bit_equal_to_the_witness(hip, name, max_out, score_thr):
    classes, passes, lists = case(name)
    S, cap = len(lists), 200
    cand = filled(hip, passes, classes, cap)
    out, h = run_soft(hip, cand, "linear", score_thr=score_thr, max_out=max_out)
    want, res = expected_pack(len(h), lists, cap, "linear", score_thr=score_thr, max_out=max_out)
    full = res if max_out == 0 else expected_pack(len(h), lists, cap, "linear", score_thr=score_thr, max_out=0)[1]
    decayed, dropped, reordered = facts_of(full)
    assert decayed, "no score was decayed: the case shows nothing"
    assert dropped, "no candidate was dropped under score_thr: the case shows nothing"
    assert reordered, "the pick order is the plain score order: the case shows nothing"
    assert max_out == 0 or any(len(f[0]) > max_out for f in full), "max_out cuts no list: the case shows nothing"
    for r, f in zip(res, full):      # max_out cuts the pick sequence, it does not change it
        assert len(r[0]) == (len(f[0]) if max_out == 0 else min(max_out, len(f[0]))) and same_bits(r[0], f[0][:len(r[0])])
    if name.startswith("S33"):
        assert [len(r[0]) for r in res[12:15]] == [0, 0, 0] and [r[2] for r in out[12:15]] == [0, 0, 0], "the image without rows"
    assert np.array_equal(h, want), np.flatnonzero(h != want)[:8]
    for (d, t, c), r in zip(out, res):
        assert same_bits(d, r[0]) and c == len(r[4])


def test_equal_probs_in_two_passes_go_to_the_pass_added_first(hip):
    """The same forward added twice: every candidate has a twin with the same box and the same prob in the other pass.  The tie
    goes to the pass added first; its twin, at overlap 1, decays to exactly 0 and is dropped."""
    p = Pass(0, [40], seed=11)
    lists = lists_of([p, p], [2])
    cand = filled(hip, [p, p], [2], 100)
    out, h = run_soft(hip, cand, "linear", score_thr=0.01)
    want, res = expected_pack(len(h), lists, 100, "linear", score_thr=0.01)
    d, slots, decays, gap, c = res[0]
    assert gap == 0.0, "no pick of the witness saw two equal scores"
    assert len(d) > 5 and np.all(slots < 40), "a tie went to the later pass in the witness"
    assert np.array_equal(h, want), np.flatnonzero(h != want)[:8]
    assert np.all(out[0][1] >> 24 == 0)


@pytest.mark.parametrize("name", list(CASES) + ["dense300"])
def test_gaussian_picks_are_exact_and_scores_within_the_derived_allowance(hip, name, capsys):
    if name == "dense300":      # 300 candidates in 40 clusters
        rng = np.random.default_rng(77)
        m = rng.integers(0, 40, 300)
        b = np.stack([200 * (m % 8) + 20 + rng.integers(-6, 7, 300), 200 * (m // 8) + 20 + rng.integers(-6, 7, 300),
                      rng.choice([28, 32, 36, 48], 300), rng.choice([28, 32, 36, 48], 300)], 1).astype(np.float64)
        classes, passes = [1], [Pass(0, [300], ncls=2, hw=BIG, seed=13, boxes=lambda n, r: b)]
        lists = lists_of(passes, classes)
    else:
        classes, passes, lists = case(name)
    S, cap = len(lists), 320
    cand = filled(hip, passes, classes, cap)
    worst = 0.0
    for sigma, max_out in ((0.5, 0), (0.25, 7)):
        out, h = run_soft(hip, cand, "gaussian", sigma=sigma, score_thr=0.001, max_out=max_out)
        want, res = expected_pack(len(h), lists, cap, "gaussian", sigma=sigma, score_thr=0.001, max_out=max_out)
        gap = min(r[3] for r in res)
        assert gap > 1e-9, f"min_gap {gap}: a last-bit difference of exp could turn a pick of this input"
        if max_out == 0:
            decayed, dropped, reordered = facts_of(res)
            assert decayed and reordered, "the case shows nothing"
        hdr, dets, tags = pack_views(h, S, cap)
        whdr, wdets, wtags = pack_views(want, S, cap)
        assert np.array_equal(hdr, whdr), "counts, header, table"
        assert np.array_equal(tags, wtags), "the picks, in order"
        assert np.array_equal(dets[:, :4].view(np.uint64), wdets[:, :4].view(np.uint64)), "boxes bit for bit, poison past every count"
        assert np.array_equal(h[16 * (S + 1) + 44 * S * cap:], want[16 * (S + 1) + 44 * S * cap:])
        for s, r in enumerate(res):
            D = len(r[0])
            got, ref = dets[s * cap:s * cap + D, 4], r[0][:, 4]
            assert np.all(dets[s * cap + D:(s + 1) * cap, 4].view(np.uint64) == 0xFFFFFFFFFFFFFFFF)
            if D:
                worst = max(worst, float(ulps(got, ref).max()))
                assert np.all(np.abs(got - ref) <= 4 * D * 2.0 ** -52 * np.abs(ref)), (s, D, float(ulps(got, ref).max()))
    with capsys.disabled():
        print(f"\n[soft gaussian {name}] largest score difference against the witness: {worst:.2f} ulp")


# ---- nothing overlaps: the hard merge's pack ----------------------------------------------------------------------------------------------------
def grid_blobs(n):
    """n disjoint 20 x 20 boxes on a 50-column grid as plain-stage blobs with zero regression at ratio 1."""
    i = np.arange(n)
    x, y = 10.0 + 40 * (i % 50), 10.0 + 40 * (i // 50)
    props = np.stack([np.zeros(n), x, y, x + 20, y + 20, np.zeros(n)], 1).astype(np.float32)
    cls_pred = np.zeros((n, 2), np.float32)
    cls_pred[:, 1] = np.random.default_rng(5).permutation(np.linspace(-2, 2, n))
    return np.zeros((n, 8), np.float32), cls_pred, props


@pytest.mark.parametrize("method", ["linear", "gaussian"])
def test_boxes_that_overlap_nothing_give_the_hard_merges_pack(hip, method):
    n = 300
    kw = dict(cls_id=2, bbox_mean=(0, 0, 0, 0), bbox_std=STD, proposal_thr=-10.0, ratios=(1.0, 1.0), org_hw=(2000, 2100), nms_overlap=0.5)
    cand = hip.Candidates(2, n + 10)
    blobs = [dev(b) for b in grid_blobs(n)]
    cand.add(*blobs, 1, [kw, dict(kw, cls_id=1)])
    nbytes = hip.lib().mscnn_detections_multi_pack_bytes(2, 2 * (n + 10))
    hard, h0 = cand.merge(raw_pack=True, pack=torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda"))
    soft, h1 = run_soft(hip, cand, method)
    assert len(hard[0][0]) == n and len(hard[1][0]) == n and not np.array_equal(hard[0][1], np.arange(n))
    assert np.array_equal(h0, h1), np.flatnonzero(h0 != h1)[:8]


# ---- the register / streaming boundary ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4096, 4097])
def test_4096_candidates_live_in_registers_and_4097_stream_through_the_workspace(hip, n):
    half = n // 2
    passes = [Pass(0, [n - half], ncls=2, hw=BIG, seed=31, boxes=dense), Pass(1, [half], ncls=2, hw=BIG, seed=31, boxes=dense)]
    lists = lists_of(passes, [2])
    wb = hip.lib().mscnn_detections_merge_soft_workspace_bytes(1, n)
    assert (wb == 256) == (n == 4096), "the list in registers needs no workspace, the streamed one its scores and live flags"
    assert n == 4096 or wb >= 9 * n
    cand = filled(hip, passes, [2], n)
    assert cand.counts() == [[n, 0]]
    ws = torch.full((wb,), 0xA5, dtype=torch.uint8, device="cuda")      # (whatever the workspace held before)
    out, h = run_soft(hip, cand, "linear", ws=ws, score_thr=0.05, max_out=64)
    want, res = expected_pack(len(h), lists, n, "linear", score_thr=0.05, max_out=64)
    d, slots, decays, gap, c = res[0]
    assert len(d) == 64 and decays > 0 and set((slots >= n - half).tolist()) == {False, True}
    assert [int(v) for v in slots] != [int(v) for v in sw.hard_order(c)[:64]], "the first 64 picks are the 64 best scores: nothing decayed in time"
    assert np.array_equal(h, want), np.flatnonzero(h != want)[:8]


# ---- an overflowed list ---------------------------------------------------------------------------------------------------------------------------
def test_an_overflowed_list_reports_its_rows_and_leaves_its_slot_alone(hip):
    classes, passes, lists = case("S4_two_passes")
    cap = 129                                    # image 0: 65 + 63 = 128 rows fit, image 1: 64 + 66 = 130 do not
    cand = filled(hip, passes, classes, cap)
    assert [c[1] for c in cand.counts()] == [0, 0, 1, 1]
    pack = torch.full((hip.lib().mscnn_detections_multi_pack_bytes(4, 4 * cap),), 0xFF, dtype=torch.uint8, device="cuda")
    out, h = run_soft(hip, cand, "linear", pack=pack, score_thr=0.05)
    want, res = expected_pack(len(h), lists, cap, "linear", score_thr=0.05)
    assert res[2] is None and res[3] is None and out[2] == (None, None, 130) and out[3] == (None, None, 130)
    hdr = pack_views(h, 4, cap)[0]
    assert hdr[3].tolist() == [-1, 130, 2 * cap, 0] and hdr[4].tolist() == [-1, 130, 3 * cap, 0]
    table = 16 * 5
    assert guarded.all_poison(pack[table + 40 * 2 * cap:table + 40 * 4 * cap]), "rows of the overflowed lists"
    assert guarded.all_poison(pack[table + 40 * 4 * cap + 4 * 2 * cap:table + 44 * 4 * cap]), "tags of the overflowed lists"
    assert np.array_equal(h, want), np.flatnonzero(h != want)[:8]


# ---- the buffer contract ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def arena(hip, monkeypatch):
    a = guarded.Arena("cuda")
    monkeypatch.setattr(hip, "torch", guarded.GuardedTorch(torch, a))
    yield a
    torch.cuda.synchronize()
    a.check()


@pytest.mark.parametrize("cap", [200, 4100])
def test_buffer_contract_of_the_soft_merge(hip, arena, cap):
    """The candidate buffer, the workspace and the pack between guard bands (both paths: at 4100 slots image 0's list is full and
    streams through the workspace): guards intact, the candidate buffer unwritten, of the pack exactly the witness's bytes;
    unaligned bases are refused before any launch."""
    if cap == 200:
        classes, passes, lists = case("S4_two_passes")
    else:
        classes = [2]
        passes = [Pass(0, [2050, 40], ncls=2, hw=BIG, seed=43, boxes=dense), Pass(1, [2050, 30], ncls=2, hw=BIG, seed=43, boxes=dense)]
        lists = lists_of(passes, classes)
    S = len(lists)
    cand = filled(hip, passes, classes, cap, arena)
    assert not arena.record(cand.buf).is_input
    nbytes = hip.lib().mscnn_detections_multi_pack_bytes(S, S * cap)
    wb = hip.lib().mscnn_detections_merge_soft_workspace_bytes(S, cap)
    pack = arena.alloc(nbytes, torch.uint8)
    ws = arena.alloc(wb, torch.uint8)
    before = cand.buf.clone()
    out, h = run_soft(hip, cand, "linear", pack=pack, ws=ws, score_thr=0.05)
    torch.cuda.synchronize()
    arena.check()
    assert torch.equal(cand.buf, before), "the op wrote the candidate buffer"
    want, res = expected_pack(len(h), lists, cap, "linear", score_thr=0.05)
    assert facts_of(res) == (True, True, True) and (cap == 200 or len(res[0][4]) == 4100)
    assert np.array_equal(h, want), np.flatnonzero(h != want)[:8]
    assert guarded.all_poison(ws) == (cap == 200), "a list in registers leaves the workspace alone"
    # unaligned bases and a short workspace: refused, nothing written
    L = hip.lib()
    ov = (hip.C.c_double * S)(*([OVERLAP] * S))
    sp = hip.C.byref(hip.SoftNmsParams(1, 0.5, 0.05, 0))
    off = arena.offset_view(cand.buf, 8)
    pack2 = arena.alloc(nbytes + 16, torch.uint8)
    ws2 = arena.alloc(wb + 16, torch.uint8)
    for c_, w_, p_, what in ((off, ws2, pack2, "cand"), (cand.buf, ws2[8:], pack2, "workspace"), (cand.buf, ws2, pack2[8:], "pack_dev")):
        assert L.mscnn_detections_merge_soft_fwd(ov, sp, S, hip._dev(c_), cap, hip._dev(p_), hip._dev(w_), hip.C.c_size_t(wb), hip._stream()) != 0
        assert f"detections_merge_soft: {what} must be 16-byte aligned" in L.mscnn_last_error().decode()
    assert L.mscnn_detections_merge_soft_fwd(ov, sp, S, hip._dev(cand.buf), cap, hip._dev(pack2), hip._dev(ws2), hip.C.c_size_t(wb - 1),
                                             hip._stream()) == 3      # MSCNN_ERR_WORKSPACE
    assert f"workspace {wb - 1} < {wb}" in L.mscnn_last_error().decode()
    torch.cuda.synchronize()
    assert guarded.all_poison(pack2) and guarded.all_poison(ws2) and torch.equal(cand.buf, before)


# ---- the vote behind it ---------------------------------------------------------------------------------------------------------------------------
def test_the_vote_runs_on_the_soft_pack_unchanged(hip):
    classes, passes, lists = case("S4_two_passes")
    cap = 200
    cand = filled(hip, passes, classes, cap)
    out, h = run_soft(hip, cand, "linear", score_thr=0.05, vote_thr=0.5)
    want, res = expected_pack(len(h), lists, cap, "linear", score_thr=0.05)
    _, dets, _ = pack_views(want, len(lists), cap)
    moved = 0
    for s, (d, slots, decays, gap, c) in enumerate(res):
        voted, who = vw.vote(d, c, 0.5)
        assert np.array_equal(voted[:, 4].view(np.uint64), d[:, 4].view(np.uint64))
        moved += int(np.count_nonzero(np.any(voted[:, :4] != d[:, :4], 1)))
        dets[s * cap:s * cap + len(d)] = voted
    assert moved >= 3, "the vote moved no box: the case shows nothing"
    assert np.array_equal(h, want), np.flatnonzero(h != want)[:8]


# ---- Net level ----------------------------------------------------------------------------------------------------------------------------------
def frame_u8(h, w, seed):
    x = synth.frame(h, w, seed=seed, org_hw=(h, w))[0].transpose(1, 2, 0)[:, :, ::-1] + np.array([123.0, 117.0, 104.0])
    return np.ascontiguousarray(np.clip(np.round(x), 0, 255).astype(np.uint8))


def test_net_soft_nms_is_the_op_in_place_of_the_merge_and_off_again_the_merge_alone(hip):
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

    def flat(res):
        return b"".join(np.ascontiguousarray(a).tobytes() for seg in res[0][0] for a in seg) + repr(res[1]).encode()

    assert n.get_soft_nms() is None
    (never, cands0), _ = run(False)                       # before the setting was ever touched
    n.set_soft_nms("linear", score_thr=0.05, max_out=50)
    assert n.get_soft_nms() == dict(method="linear", sigma=0.5, score_thr=0.05, max_out=50)
    (soft, cands), fw = run(True)
    n.set_soft_nms("linear", score_thr=0.05, max_out=50)
    n.set_box_voting(0.5)
    (soft_voted, _), _ = run(False)
    n.set_box_voting(None)
    n.set_soft_nms(None)
    (plain, cands2), _ = run(False)
    assert cands == cands2 == cands0 and flat((never, cands0)) == flat((plain, cands2)), "off again: what it always returned"
    # the same blobs through the ops
    cand = hip.Candidates(len(classes), NET_CAP)
    for blobs, p, flipped in fw:
        segs = [dict(cls_id=c, bbox_mean=(0, 0, 0, 0), bbox_std=STD, proposal_thr=-10.0, ratios=p["ratios"], org_hw=p["org_hw"], nms_overlap=0.5)
                for c in classes]
        cand.add(*[dev(b) for b in blobs], 1, segs, views=[FLIP] if flipped else None)
    ref_plain = cand.merge()
    ref_soft = cand.merge_soft("linear", score_thr=0.05, max_out=50)
    ref_voted = cand.merge_soft("linear", score_thr=0.05, max_out=50, vote_thr=0.5)
    differs = 0
    for ci in range(len(classes)):
        for got, ref in ((plain, ref_plain), (soft, ref_soft), (soft_voted, ref_voted)):
            dets, pas, row = got[0][ci]
            assert same_bits(dets, ref[ci][0]) and np.array_equal((pas << 24) | row, ref[ci][1]) and cands[0][ci] == ref[ci][2], ci
        differs += len(soft[0][ci][0]) != len(plain[0][ci][0]) or not same_bits(soft[0][ci][0], plain[0][ci][0])
    assert differs >= 1, "Soft-NMS returned the hard NMS's rows on this net: the case shows nothing"
