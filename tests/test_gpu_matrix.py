"""Matrix NMS over the merged candidates on the GPU: mscnn_detections_merge_matrix_fwd through the HIP ABI on synthetic, seeded
candidate lists, Net.set_matrix_nms on a reduced deploy, and the driver's --matrix-nms.  No pin on the reference, whose scripts
neither merge nor decay a score: the check is tests/matrix_witness.py.

LINEAR is IEEE operations only and min / max of doubles are exact in any order: the whole pack -- header, table, rows, tags, and every
byte the op must leave alone (the pack starts as 0xFF poison) -- is compared BYTE FOR BYTE with the pack the witness describes.
GAUSSIAN calls exp ONCE per candidate (OCML's on the device, numpy's in the witness): boxes, tags and counts are exact, the scores lie
within 4 * 2^-52 relative -- Soft-NMS's own per-decay allowance (two exp results of at most 1 ulp each and two roundings of the
product), and a candidate has one decay here.  The order is exact under the ASSERTED condition that the witness's min_gap > 1e-9.

Each case first shows ON THE WITNESS'S OWN RESULT, wherever the list is long enough, matrix_witness.matrix_facts (a) to (e): a score
was decayed, a candidate fell under score_thr, the output order is not the sorted order, the compensation mattered, and the scores are
not Soft-NMS's.

Shapes, the smallest at which the kernels can go wrong: 1 and 2 candidates, the edges of a wave (63 / 64 / 65) and of the 256-row
tile (255 / 256 / 257), 1000 (four column blocks, row splits that hold zero, one and two tiles), 4032 / 4033 slots (the one-pass
sort's last size, the tiled sort's first), 8200 (the tiled sort's 16384 keys, 33 column blocks over 8 row splits), an empty and an
overflowed list, 33 segments (over the 32 of a launch).  The lists are test_gpu_soft's constructions (clusters of about five boxes
on a 16-column grid)."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import guarded                                   # noqa: E402
import matrix_witness as xw                      # noqa: E402
import merge_witness as mw                       # noqa: E402
import test_gpu_soft as gs                       # noqa: E402  (Pass, dense, lists_of, filled, pack_views: the lists' construction)
import vote_witness as vw                        # noqa: E402
from mscnn_amd import kitti, net as mnet, synth, zoo   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = 0.05
Pass, dense, BIG, FLIP, STD = gs.Pass, gs.dense, gs.BIG, gs.FLIP, gs.STD
same_bits, pack_views, dev = gs.same_bits, gs.pack_views, gs.dev


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X: torch.cuda.is_available() is False")
    from mscnn_amd import hipapi
    hipapi.lib()
    return hipapi


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
        d, pas, row, cands, slots, info, cand = xw.matrix_segment(passes, xw.METHODS[method], **kw)
        hdr[1 + s] = [len(d), n, s * cap, 0]
        dets[s * cap:s * cap + len(d)] = d
        tags[s * cap:s * cap + len(d)] = (pas.astype(np.int32) << 24) | row
        res.append((d, slots, info, cand))
    return want, res


def facts_of(res, score_thr, rerun=False):
    """matrix_witness.matrix_facts (a) .. (e) over all segments of a case; rerun: res was made with a max_out or gaussian, so the
    linear witness runs again without."""
    f = np.zeros(5, bool)
    for r in res:
        if r is not None and len(r[3]):
            d, slots, info = xw.matrix(r[3], xw.LINEAR, score_thr=score_thr) if rerun else r[:3]
            f |= np.array(xw.matrix_facts(r[3], d, slots, info, score_thr))
    return tuple(bool(v) for v in f)


def run_matrix(hip, cand, method, pack=None, ws=None, **kw):
    """The op on a 0xFF-poisoned pack: (merge_matrix's result, the pack's bytes)."""
    if pack is None:
        pack = torch.full((hip.lib().mscnn_detections_multi_pack_bytes(cand.S, cand.S * cand.cap),), 0xFF, dtype=torch.uint8, device="cuda")
    return cand.merge_matrix(method, raw_pack=True, pack=pack, ws=ws, **kw)


_cache = {}


def one_list(n, seed=7):
    """(classes, passes, lists) of ONE list of n candidates from two forwards (one for n = 1), built once per module."""
    if (n, seed) not in _cache:
        half = n // 2
        passes = [Pass(0, [n - half], ncls=2, hw=BIG, seed=seed, boxes=dense)] + ([Pass(1, [half], ncls=2, hw=BIG, seed=seed, boxes=dense)] if half else [])
        _cache[(n, seed)] = ([2], passes, gs.lists_of(passes, [2]))
    return _cache[(n, seed)]


def check_linear(hip, classes, passes, lists, cap, facts=True, **kw):
    cand = gs.filled(hip, passes, classes, cap)
    out, h = run_matrix(hip, cand, "linear", **kw)
    want, res = expected_pack(len(h), lists, cap, "linear", **kw)
    if facts:
        assert facts_of(res, kw.get("score_thr", 0.001), bool(kw.get("max_out"))) == (True,) * 5, "the case shows nothing: facts (a) .. (e)"
    assert np.array_equal(h, want), np.flatnonzero(h != want)[:8]
    for (d, t, c), r in zip(out, res):
        assert r is None or (same_bits(d, r[0]) and c == len(r[3]))
    return res, h


# ---- linear, the pack byte for byte --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_linear_is_bit_equal_to_the_witness_at_the_tile_edges(hip, n):
    classes, passes, lists = one_list(n)
    res, _ = check_linear(hip, classes, passes, lists, n + 3, facts=n >= 63, score_thr=THR)
    assert len(res[0][3]) == n


def fixed_boxes(b):
    return lambda n, rng: np.asarray(b, np.float64)[:n]


def test_two_disjoint_boxes_keep_their_scores_and_exact_duplicates_take_the_skip_rule(hip):
    p = Pass(0, [2], ncls=2, hw=BIG, seed=3, boxes=fixed_boxes([[100, 100, 40, 40], [900, 700, 40, 40]]))
    res, _ = check_linear(hip, [2], [p], gs.lists_of([p], [2]), 5, facts=False, score_thr=0.0)
    d, slots, info, cand = res[0]
    assert len(d) == 2 and info["decayed"] == 0 and info["comp"].tolist() == [0.0, 0.0]
    # the same one-row forward added twice and three times: c = 1 from the second copy on; the third's terms of the second are
    # skipped (1 - c is not > 0), the first copy's term is an exact 0
    q = Pass(0, [1], ncls=2, hw=BIG, seed=4, boxes=fixed_boxes([[100, 100, 40, 40]]))
    for copies in (2, 3):
        res, _ = check_linear(hip, [2], [q] * copies, gs.lists_of([q] * copies, [2]), 4, facts=False, score_thr=0.0)
        d, slots, info, cand = res[0]
        assert info["comp"].tolist() == [0.0] + [1.0] * (copies - 1) and info["scores"][1:].tolist() == [0.0] * (copies - 1)
        assert slots.tolist() == list(range(copies)) and d[0, 4] > 0, "the earlier add first, in the sort and among the equal zeros"


@pytest.mark.parametrize("cap", [4032, 4033])
def test_full_lists_on_both_sort_paths(hip, cap):
    classes, passes, lists = one_list(cap, seed=31)
    res, h = check_linear(hip, classes, passes, lists, cap, score_thr=THR)
    assert pack_views(h, 1, cap)[0][1].tolist()[1:] == [cap, 0, 0] and len(res[0][0]) > 1000


def test_long_list_through_the_tiled_sort(hip):
    n = 8200
    classes, passes, lists = one_list(n, seed=37)
    res, _ = check_linear(hip, classes, passes, lists, n, score_thr=THR)
    slots = res[0][1]
    assert len(slots) > 2000 and set((slots >= n - n // 2).tolist()) == {False, True}


def test_an_empty_and_an_overflowed_list_between_two_good_ones(hip):
    # 4 images x 1 class: 130 rows, none, 205 (over the 200 slots), 140
    passes = [Pass(0, [65, 0, 100, 70], ncls=2, hw=BIG, seed=41, boxes=dense), Pass(1, [65, 0, 105, 70], ncls=2, hw=BIG, seed=41, boxes=dense)]
    lists = gs.lists_of(passes, [2])
    cap = 200
    cand = gs.filled(hip, passes, [2], cap)
    assert [c[1] for c in cand.counts()] == [0, 0, 1, 0]
    pack = torch.full((hip.lib().mscnn_detections_multi_pack_bytes(4, 4 * cap),), 0xFF, dtype=torch.uint8, device="cuda")
    out, h = run_matrix(hip, cand, "linear", pack=pack, score_thr=THR)
    want, res = expected_pack(len(h), lists, cap, "linear", score_thr=THR)
    assert res[2] is None and out[2] == (None, None, 205) and out[1][2] == 0 and len(out[1][0]) == 0
    hdr = pack_views(h, 4, cap)[0]
    assert hdr[2].tolist() == [0, 0, cap, 0] and hdr[3].tolist() == [-1, 205, 2 * cap, 0]
    table = 16 * 5
    assert guarded.all_poison(pack[table + 40 * cap:table + 40 * 3 * cap]), "rows of the empty and the overflowed list"
    assert guarded.all_poison(pack[table + 40 * 4 * cap + 4 * cap:table + 40 * 4 * cap + 4 * 3 * cap]), "their tags"
    assert facts_of(res, THR) == (True,) * 5
    assert np.array_equal(h, want), np.flatnonzero(h != want)[:8]


def test_33_segments_of_unequal_lengths_cross_the_launch_boundary(hip):
    rows0 = [9, 70, 12, 8, 0, 90, 12, 7, 80, 9, 12]
    rows1 = [8, 12, 70, 9, 0, 10, 80, 9, 12, 70, 9]
    passes = [Pass(0, rows0, seed=5, hw=BIG, boxes=dense), Pass(1, rows1, ratios=(1.5, 1.25), view=FLIP, hw=BIG, seed=5, boxes=dense)]
    lists = gs.lists_of(passes, [1, 2, 3])
    assert len(lists) == 33
    res, h = check_linear(hip, [1, 2, 3], passes, lists, 170, score_thr=THR)
    assert [len(r[0]) for r in res[12:15]] == [0, 0, 0] and len(res[32][0]) > 0, "the image without rows; the segment of the second launch"


# ---- score_thr, max_out, ties --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_out,score_thr", [(0, 0.3), (1, THR), (7, THR), (100000, THR)])
def test_score_thr_cuts_inside_the_list_and_max_out_cuts_the_order(hip, max_out, score_thr):
    classes, passes, lists = one_list(257)
    res, _ = check_linear(hip, classes, passes, lists, 300, score_thr=score_thr, max_out=max_out)
    full = xw.matrix(res[0][3], xw.LINEAR, score_thr=score_thr)
    D = len(res[0][0])
    assert 1 < len(full[0]) < 257, "score_thr cuts nothing, or everything"
    assert D == (len(full[0]) if max_out == 0 else min(max_out, len(full[0]))) and same_bits(res[0][0], full[0][:D])


def test_equal_probs_in_two_passes_go_to_the_pass_added_first(hip):
    """The same forward added twice: every candidate has a twin with the same box and prob in the other pass.  The tie goes to the
    pass added first in the sort; its twin, at overlap 1, decays to exactly 0 -- and the zeros come out in sorted order."""
    p = Pass(0, [40], ncls=2, hw=BIG, seed=11, boxes=dense)
    lists = gs.lists_of([p, p], [2])
    res, h = check_linear(hip, [2], [p, p], lists, 100, facts=False, score_thr=0.0)
    d, slots, info, cand = res[0]
    order = info["order"]
    assert np.all(order[0::2] < 40) and np.array_equal(order[1::2], order[0::2] + 40), "the sort: each first-pass row, then its twin"
    assert np.all(info["scores"][1::2] == 0.0) and len(d) == 80
    zeros = slots[d[:, 4] == 0.0]
    assert len(zeros) >= 40 and np.array_equal(zeros[zeros >= 40], order[1::2]), "equal scores: the lower sorted position first"
    tags = pack_views(h, 1, 100)[2][:80]
    assert np.array_equal(tags >> 24, (slots >= 40).astype(np.int32))


# ---- gaussian ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.5, 0.1])
@pytest.mark.parametrize("n", [257, 1000])
def test_gaussian_order_is_exact_and_scores_within_one_decays_allowance(hip, n, sigma, capsys):
    classes, passes, lists = one_list(n)
    cap = n + 3
    cand = gs.filled(hip, passes, classes, cap)
    out, h = run_matrix(hip, cand, "gaussian", sigma=sigma, score_thr=THR)
    want, res = expected_pack(len(h), lists, cap, "gaussian", sigma=sigma, score_thr=THR)
    d, slots, info, c = res[0]
    assert info["min_gap"] > 1e-9, f"min_gap {info['min_gap']}: a last-bit difference of exp could turn the order of this input"
    assert info["decayed"] > 0 and len(d) < n and facts_of(res, THR, True) == (True,) * 5
    hdr, dets, tags = pack_views(h, 1, cap)
    whdr, wdets, wtags = pack_views(want, 1, cap)
    assert np.array_equal(hdr, whdr), "count, header, table"
    assert np.array_equal(tags, wtags), "the order"
    assert np.array_equal(dets[:, :4].view(np.uint64), wdets[:, :4].view(np.uint64)), "boxes bit for bit, poison past the count"
    D = len(d)
    assert np.all(dets[D:, 4].view(np.uint64) == 0xFFFFFFFFFFFFFFFF)
    got, ref = dets[:D, 4], d[:, 4]
    worst = float(gs.ulps(got, ref).max())
    with capsys.disabled():
        print(f"\n[matrix gaussian n={n} sigma={sigma}] largest score difference against the witness: {worst:.2f} ulp")
    assert np.all(np.abs(got - ref) <= 4 * 2.0 ** -52 * np.abs(ref)), worst


# ---- the vote behind it --------------------------------------------------------------------------------------------------------------------------
def test_the_vote_runs_on_the_matrix_pack_unchanged(hip):
    classes, passes, lists = gs.case("S4_two_passes")
    cap = 200
    cand = gs.filled(hip, passes, classes, cap)
    out, h = run_matrix(hip, cand, "linear", score_thr=THR, vote_thr=0.5)
    want, res = expected_pack(len(h), lists, cap, "linear", score_thr=THR)
    _, dets, _ = pack_views(want, len(lists), cap)
    moved = 0
    for s, (d, slots, info, c) in enumerate(res):
        voted, who = vw.vote(d, c, 0.5)
        assert np.array_equal(voted[:, 4].view(np.uint64), d[:, 4].view(np.uint64))
        moved += int(np.count_nonzero(np.any(voted[:, :4] != d[:, :4], 1)))
        dets[s * cap:s * cap + len(d)] = voted
    assert moved >= 3, "the vote moved no box: the case shows nothing"
    assert np.array_equal(h, want), np.flatnonzero(h != want)[:8]


# ---- determinism ---------------------------------------------------------------------------------------------------------------------------------
def test_the_same_call_twice_gives_the_same_bytes(hip):
    classes, passes, lists = one_list(1000)
    cand = gs.filled(hip, passes, classes, 1003)
    for method in ("linear", "gaussian"):
        _, h0 = run_matrix(hip, cand, method, score_thr=THR)
        _, h1 = run_matrix(hip, cand, method, score_thr=THR)
        assert np.array_equal(h0, h1) and pack_views(h0, 1, 1003)[0][1][0] > 100, method


# ---- the buffer contract -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def arena(hip, monkeypatch):
    a = guarded.Arena("cuda")
    monkeypatch.setattr(hip, "torch", guarded.GuardedTorch(torch, a))
    yield a
    torch.cuda.synchronize()
    a.check()


@pytest.mark.parametrize("cap", [200, 4100])
def test_buffer_contract_of_the_matrix_merge(hip, arena, cap):
    """The candidate buffer, the workspace and the pack between guard bands (both sort paths: 4100 slots go list after list through
    the tiled sort, image 0's list full): guards intact, the candidate buffer unwritten, of the pack exactly the witness's bytes;
    unaligned bases and a short workspace are refused before any launch."""
    if cap == 200:
        classes, passes, lists = gs.case("S4_two_passes")
    else:
        classes = [2]
        passes = [Pass(0, [2050, 40], ncls=2, hw=BIG, seed=43, boxes=dense), Pass(1, [2050, 30], ncls=2, hw=BIG, seed=43, boxes=dense)]
        lists = gs.lists_of(passes, classes)
    S = len(lists)
    cand = gs.filled(hip, passes, classes, cap, arena)
    nbytes = hip.lib().mscnn_detections_multi_pack_bytes(S, S * cap)
    wb = hip.lib().mscnn_detections_merge_matrix_workspace_bytes(S, cap)
    pack = arena.alloc(nbytes, torch.uint8)
    ws = arena.alloc(wb, torch.uint8)
    before = cand.buf.clone()
    out, h = run_matrix(hip, cand, "linear", pack=pack, ws=ws, score_thr=THR)
    torch.cuda.synchronize()
    arena.check()
    assert torch.equal(cand.buf, before), "the op wrote the candidate buffer"
    want, res = expected_pack(len(h), lists, cap, "linear", score_thr=THR)
    assert facts_of(res, THR) == (True,) * 5 and (cap == 200 or len(res[0][3]) == 4100)
    assert np.array_equal(h, want), np.flatnonzero(h != want)[:8]
    L = hip.lib()
    mp = hip.C.byref(hip.MatrixNmsParams(1, 0.5, THR, 0))
    off = arena.offset_view(cand.buf, 8)
    pack2 = arena.alloc(nbytes + 16, torch.uint8)
    ws2 = arena.alloc(wb + 16, torch.uint8)
    for c_, w_, p_, what in ((off, ws2, pack2, "cand"), (cand.buf, ws2[8:], pack2, "workspace"), (cand.buf, ws2, pack2[8:], "pack_dev")):
        assert L.mscnn_detections_merge_matrix_fwd(mp, S, hip._dev(c_), cap, hip._dev(p_), hip._dev(w_), hip.C.c_size_t(wb), hip._stream()) != 0
        assert f"detections_merge_matrix: {what} must be 16-byte aligned" in L.mscnn_last_error().decode()
    assert L.mscnn_detections_merge_matrix_fwd(mp, S, hip._dev(cand.buf), cap, hip._dev(pack2), hip._dev(ws2), hip.C.c_size_t(wb - 1),
                                               hip._stream()) == 3      # MSCNN_ERR_WORKSPACE
    assert f"workspace {wb - 1} < {wb}" in L.mscnn_last_error().decode()
    torch.cuda.synchronize()
    assert guarded.all_poison(pack2) and guarded.all_poison(ws2) and torch.equal(cand.buf, before)


# ---- Net level -----------------------------------------------------------------------------------------------------------------------------------
def test_net_matrix_nms_is_the_op_in_place_of_the_merge_and_off_again_the_merge_alone(hip):
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=96, width=320))
    synth.load_into(n, "mid")
    img = gs.frame_u8(375, 1242, 41)
    classes = [2, 3]

    def run(keep_blobs):
        """A frame and its mirror, merged: (detect_merge_end's result, the forwards' blobs and params)."""
        fw = []
        n.detect_merge_begin(1, len(classes), gs.NET_CAP)
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

    assert n.get_matrix_nms() is None
    (never, cands0), _ = run(False)                       # before the setting was ever touched
    n.set_matrix_nms("linear", score_thr=THR, max_out=50)
    assert n.get_matrix_nms() == dict(method="linear", sigma=0.5, score_thr=THR, max_out=50)
    with pytest.raises(mnet.NetError, match="while Matrix NMS is on"):
        n.set_soft_nms("linear")
    (mat, cands), fw = run(True)
    n.set_box_voting(0.5)
    (mat_voted, _), _ = run(False)
    n.set_box_voting(None)
    n.set_matrix_nms(None)
    (plain, cands2), _ = run(False)
    assert cands == cands2 == cands0 and flat((never, cands0)) == flat((plain, cands2)), "off again: what it always returned"
    # the witness on the blobs of those forwards, and the ops on them
    cand = hip.Candidates(len(classes), gs.NET_CAP)
    witness = [[] for _ in classes]
    for blobs, p, flipped in fw:
        segs = [dict(cls_id=c, bbox_mean=(0, 0, 0, 0), bbox_std=STD, proposal_thr=-10.0, ratios=p["ratios"], org_hw=p["org_hw"], nms_overlap=0.5)
                for c in classes]
        cand.add(*[dev(b) for b in blobs], 1, segs, views=[FLIP] if flipped else None)
        for ci, c in enumerate(classes):
            rows, ids = mw.plain_rows(*blobs, c, bbox_stds=STD, proposal_thr=-10.0, ratios=p["ratios"], org_hw=p["org_hw"])
            witness[ci].append((mw.apply_view(rows, np.float32(p["org_hw"][1]), FLIP if flipped else None), ids))
    ref_voted = cand.merge_matrix("linear", score_thr=THR, max_out=50, vote_thr=0.5)
    differs = 0
    for ci in range(len(classes)):
        d, pas, row, ncand, slots, info, _ = xw.matrix_segment(witness[ci], xw.LINEAR, score_thr=THR, max_out=50)
        dets, gpas, grow = mat[0][ci]
        assert len(d) > 5 and same_bits(dets, d) and np.array_equal(gpas, pas) and np.array_equal(grow, row) and cands[0][ci] == ncand, ci
        vdets, vpas, vrow = mat_voted[0][ci]
        assert same_bits(vdets, ref_voted[ci][0]) and np.array_equal((vpas << 24) | vrow, ref_voted[ci][1]), ci
        differs += len(dets) != len(plain[0][ci][0]) or not same_bits(dets, plain[0][ci][0])
    assert differs >= 1, "Matrix NMS returned the hard NMS's rows on this net: the case shows nothing"


def test_driver_with_matrix_nms_writes_the_witness_rows(hip, tmp_path, monkeypatch, capsys):
    spec = importlib.util.spec_from_file_location("run_mscnn_detection", os.path.join(ROOT, "tools", "run_mscnn_detection.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    deploy = tmp_path / "deploy.prototxt"
    deploy.write_text(zoo.prototxt("kitti_car/mscnn-7s-576", height=96, width=320))
    frames = []
    end = mnet.Net.detect_merge_end

    def recording_end(self, *args, **kw):      # the one forward of the frame is still in the net's blobs
        R = self.blob_shape("proposals_score")[0]
        frames.append([self.get_blob(b).reshape(R, -1).copy() for b in ("bbox_pred", "cls_pred", "proposals_score")])
        return end(self, *args, **kw)

    monkeypatch.setattr(mnet.Net, "detect_merge_end", recording_end)
    out = tmp_path / "out"
    assert drv.main(["--prototxt", str(deploy), "--synthetic", "2", "--out", str(out), "--comp-id", "t", "--cls-ids", "2",
                     "--matrix-nms", "linear", "--soft-thr", str(THR), "--max-dets", "40"]) == 0
    capsys.readouterr()
    assert len(frames) == 2
    per_frame = []
    for blobs in frames:
        rows, ids = mw.plain_rows(*blobs, 2, bbox_stds=STD, proposal_thr=-10.0, ratios=(96 / 375.0, 320 / 1242.0), org_hw=(375, 1242))
        d = xw.matrix_segment([(rows, ids)], xw.LINEAR, score_thr=THR, max_out=40)[0]
        assert 5 < len(d) <= 40
        per_frame.append(d)
    kitti.write_detections_dlm(str(tmp_path / "want.txt"), per_frame)
    assert (out / "t_car.txt").read_bytes() == (tmp_path / "want.txt").read_bytes()
