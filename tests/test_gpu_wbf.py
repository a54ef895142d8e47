"""Weighted boxes fusion over the merged candidates on the GPU: mscnn_detections_merge_wbf_fwd through the HIP ABI on synthetic, seeded
candidate lists (built as tests/test_gpu_soft.py builds them), and Net.set_wbf / detect_merge_members on a reduced deploy.  No pin on
the reference, whose scripts run one forward per image and neither merge nor fuse: the check is tests/wbf_witness.py.

The op is IEEE operations only, so the bar is bit equality, not a tolerance: the whole pack -- header, table, rows, tags, and every
byte the op must leave alone (the pack and the members buffer start as 0xFF poison) -- is compared BYTE FOR BYTE with what the witness
says the op writes, and so is the members buffer.

Each witness case first shows ON THE WITNESS'S OWN RESULT the five facts of wbf_witness.wbf_facts: a case can not pass with a hard
NMS, with NMS + vote, with a first-match instead of the argmax, or without the members / T scaling.

Shapes, the smallest at which the kernel can go wrong -- the boundaries of det_wbf.hip beside the constants they come from:
  WAVE = 64                 a wave's lanes: the waves that own a cluster take part in a step's reduction (clusters 64 | 65)
  THREADS = kWbfThreads     1024: a thread's second cluster (clusters 1024 | 1025)
  REGS = kWbfRegs           4096 = kWbfThreads * kWbfPer: a list of <= 4096 candidates keeps its fused boxes in registers, a longer
                            one reads them from the workspace (candidates 4096 | 4097; clusters past 4096 only ever streamed)
  MAXK = kMaxK              4032: the merge's one-pass sort | the tiled path's sort (cand_cap 4032 | 4033)
  SEGS = kSegsPerLaunch     32 segments per launch (the 33-segment case)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import guarded                                   # noqa: E402
import test_gpu_soft as gs                       # noqa: E402  (Pass, clustered, dense, grid_blobs, lists_of, filled, pack_views, CASES)
import wbf_witness as ww                         # noqa: E402
from mscnn_amd import net as mnet, synth, zoo   # noqa: E402

WAVE, THREADS, REGS, MAXK = 64, 1024, 4096, 4032
THR = 0.55
Pass, dense, BIG, FLIP, STD = gs.Pass, gs.dense, gs.BIG, gs.FLIP, gs.STD
same_bits, pack_views, dev = gs.same_bits, gs.pack_views, gs.dev


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X: torch.cuda.is_available() is False")
    from mscnn_amd import hipapi
    hipapi.lib()
    return hipapi


def sparse(n, rng):
    """n boxes in clusters of about one on a 64-column grid: most clusters are singletons, so the cluster count is near n."""
    m = rng.integers(0, max(1, n), n)
    xy = np.stack([120 * (m % 64) + 20, 120 * (m // 64) + 20], 1) + rng.integers(-6, 7, (n, 2))
    return np.concatenate([xy, rng.choice([14, 20, 32, 48], (n, 2))], 1).astype(np.float64)


# ---- the expectation: the poisoned pack and members buffer with what the witness says the op writes ----------------------------------------
def expected_of(nbytes, lists, cap, expected=1, **kw):
    """(the bytes a 0xFF-poisoned pack must hold after the op, those of the members buffer, the witness's result per segment (None:
    the list overflowed): (dets, first slots, members, cluster_of, min_gap, cand))."""
    S = len(lists)
    want = np.full(nbytes, 0xFF, np.uint8)
    wmem = np.full(S * cap, -1, np.int32)      # (0xFF poison)
    hdr, dets, tags = pack_views(want, S, cap)
    hdr[0] = [S, cap, S * cap, 0]
    ex = [expected] * S if isinstance(expected, int) else list(expected)
    res = []
    for s, passes in enumerate(lists):
        n = sum(len(r) for r, _ in passes)
        if n > cap:
            hdr[1 + s] = [-1, n, s * cap, 0]
            res.append(None)
            continue
        d, pas, row, cands, first, members, cluster_of, gap = ww.wbf_segment(passes, expected=ex[s], **kw)
        hdr[1 + s] = [len(d), n, s * cap, 0]
        dets[s * cap:s * cap + len(d)] = d
        tags[s * cap:s * cap + len(d)] = (pas.astype(np.int32) << 24) | row
        wmem[s * cap:s * cap + len(d)] = members
        res.append((d, first, members, cluster_of, gap, ww.candidates_of(passes)[0]))
    return want, wmem, res


def facts_of(res, expected=1, **kw):
    """wbf_witness.wbf_facts 1 .. 5 over all segments of a case (max_out is not a fact's business)."""
    kw = {k: v for k, v in kw.items() if k != "max_out"}
    f = np.zeros(5, bool)
    for r in res:
        if r is not None and len(r[5]):
            f |= np.array(ww.wbf_facts(r[5], expected=expected, **kw))
    return tuple(bool(v) for v in f)


def run_wbf(hip, cand, pack=None, ws=None, members=None, **kw):
    """The op on a 0xFF-poisoned pack and members buffer: (merge_wbf's result, the pack's bytes, the members buffer's int32)."""
    if pack is None:
        pack = torch.full((hip.lib().mscnn_detections_multi_pack_bytes(cand.S, cand.S * cand.cap),), 0xFF, dtype=torch.uint8, device="cuda")
    if members is None:
        members = torch.full((cand.S * cand.cap,), -1, dtype=torch.int32, device="cuda")
    ((out, h), mem) = cand.merge_wbf(THR, raw_pack=True, pack=pack, ws=ws, members=members, **kw)
    return out, h, members.cpu().numpy(), mem


def check(hip, classes, passes, lists, cap, facts=True, **kw):
    """The op against the witness, byte for byte; kw: skip_thr, conf, expected, max_out."""
    wkw = dict(thr=THR, skip_thr=kw.get("skip_thr", 0.0), conf_type=ww.CONF_TYPES[kw.get("conf", "avg")], max_out=kw.get("max_out", 0))
    cand = gs.filled(hip, passes, classes, cap)
    out, h, mem, per_seg = run_wbf(hip, cand, **kw)
    want, wmem, res = expected_of(len(h), lists, cap, expected=kw.get("expected", 1), **wkw)
    if facts:
        assert facts_of(res, expected=kw.get("expected", 1), **wkw) == (True,) * 5, "the case shows nothing: facts 1 .. 5"
    assert np.array_equal(h, want), np.flatnonzero(h != want)[:8]
    assert np.array_equal(mem, wmem), np.flatnonzero(mem != wmem)[:8]
    for (d, t, c), m, r in zip(out, per_seg, res):
        assert r is None or (same_bits(d, r[0]) and c == len(r[5]) and np.array_equal(m, r[2]))
    return res, h, mem


# ---- the soft tests' two cases, every parameter -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conf", ["avg", "max"])
@pytest.mark.parametrize("skip_thr", [0.05, 0.3])
@pytest.mark.parametrize("name", list(gs.CASES))
def test_the_pack_and_the_members_are_byte_equal_to_the_witness(hip, name, skip_thr, conf):
    """S4_two_passes has 128 and 130 rows per list as it stands: the facts need no more."""
    classes, passes, lists = gs.case(name)
    S, cap = len(lists), 200
    cand = gs.filled(hip, passes, classes, cap)
    for expected in (1, 2, 3):
        wkw = dict(thr=THR, skip_thr=skip_thr, conf_type=ww.CONF_TYPES[conf])
        f = facts_of([(None,) * 5 + (ww.candidates_of(l)[0],) for l in lists], expected=expected, **wkw)
        assert f[0], "no cluster of >= 2 members beside a cluster of one: the case shows nothing"
        assert f[1], "no candidate joined a cluster whose first member it does not overlap: the case shows nothing beyond NMS + vote"
        assert f[2], "no candidate chose between two clusters above thr: the argmax shows nothing"
        assert f[4], "no candidate failed skip_thr: the case shows nothing"
        # conf max with expected 1 is s_first unscaled, which DEscends in creation order by construction of the walk: fact 4 is
        # impossible there, and its negation is asserted instead
        assert f[3] == (not (conf == "max" and expected == 1)), "the output order against the creation order"
        full = None
        for max_out in (0, 1, 7):
            out, h, mem, per_seg = run_wbf(hip, cand, skip_thr=skip_thr, conf=conf, expected=expected, max_out=max_out)
            want, wmem, res = expected_of(len(h), lists, cap, expected=expected, max_out=max_out, **wkw)
            full = res if max_out == 0 else full
            assert max_out == 0 or any(len(r[0]) > max_out for r in full), "max_out cuts no list: the case shows nothing"
            for r, fr in zip(res, full):      # max_out cuts the output, it changes no kept row
                assert len(r[0]) == (len(fr[0]) if max_out == 0 else min(max_out, len(fr[0]))) and same_bits(r[0], fr[0][:len(r[0])])
                assert np.array_equal(r[2], fr[2][:len(r[0])])
            if name.startswith("S33"):
                assert [len(r[0]) for r in res[12:15]] == [0, 0, 0] and [r[2] for r in out[12:15]] == [0, 0, 0], "the image without rows"
            assert np.array_equal(h, want), np.flatnonzero(h != want)[:8]
            assert np.array_equal(mem, wmem), np.flatnonzero(mem != wmem)[:8]
            for (d, t, c), m, r in zip(out, per_seg, res):
                assert same_bits(d, r[0]) and c == len(r[5]) and np.array_equal(m, r[2])


def test_the_same_forward_added_twice_joins_every_twin_at_overlap_one(hip):
    """Every candidate has a twin with the same box and prob in the second pass.  A twin is walked right behind its original (the
    tie goes to the pass added first), whose cluster then holds a fused box; it joins SOME cluster, so members are even exactly when
    every twin follows its original into the same one -- which the witness shows first.  The tags are the first pass's; with
    expected = 2 and conf avg no cluster is marked down: every cluster has >= 2 members."""
    p = Pass(0, [40], seed=11)
    lists = gs.lists_of([p, p], [2])
    res, h, mem = check(hip, [2], [p, p], lists, 100, facts=False, skip_thr=0.0, conf="avg", expected=2)
    d, first, members, cluster_of, gap, cand = res[0]
    assert np.array_equal(cluster_of[:40], cluster_of[40:]) and np.all(cluster_of >= 0), "a twin left its original's cluster in the witness"
    assert len(d) >= 3 and np.all(members % 2 == 0) and np.all(first < 40)
    hdr, dets, tags = pack_views(h, 1, 100)
    assert np.all(tags[:len(d)] >> 24 == 0), "the tags are the first pass's"
    one = ww.wbf(cand, THR, 0.0, ww.AVG, 1)
    assert same_bits(one[0], d), "expected = 2 marked a cluster of >= 2 members down"


def test_boxes_that_overlap_nothing_are_clusters_of_one_and_the_hard_merges_pack(hip):
    n = 300
    kw = dict(cls_id=2, bbox_mean=(0, 0, 0, 0), bbox_std=STD, proposal_thr=-10.0, ratios=(1.0, 1.0), org_hw=(2000, 2100), nms_overlap=0.5)
    cand = hip.Candidates(2, n + 10)
    blobs = [dev(b) for b in gs.grid_blobs(n)]
    cand.add(*blobs, 1, [kw, dict(kw, cls_id=1)])
    nbytes = hip.lib().mscnn_detections_multi_pack_bytes(2, 2 * (n + 10))
    hard, h0 = cand.merge(raw_pack=True, pack=torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda"))
    out, h1, mem, per_seg = run_wbf(hip, cand, skip_thr=0.0, conf="avg", expected=1)
    assert len(hard[0][0]) == n and len(hard[1][0]) == n and not np.array_equal(hard[0][1], np.arange(n))
    assert np.array_equal(h0, h1), np.flatnonzero(h0 != h1)[:8]
    assert all(np.array_equal(m, np.ones(n, np.int32)) for m in per_seg), "every cluster has one member"
    assert np.all(mem.reshape(2, n + 10)[:, n:] == -1)


# ---- list lengths and cluster counts across every boundary of the implementation ----------------------------------------------------------------
_cache = {}


def one_list(n, boxes, seed=7):
    """(classes, passes, lists) of ONE list of n candidates from two forwards (one for n = 1), built once per module."""
    key = (n, boxes.__name__, seed)
    if key not in _cache:
        half = n // 2
        passes = [Pass(0, [n - half], ncls=2, hw=BIG, seed=seed, boxes=boxes)] + ([Pass(1, [half], ncls=2, hw=BIG, seed=seed, boxes=boxes)] if half else [])
        _cache[key] = ([2], passes, gs.lists_of(passes, [2]))
    return _cache[key]


@pytest.mark.parametrize("n", [1, 2, WAVE - 1, WAVE, WAVE + 1, THREADS, THREADS + 1, MAXK, MAXK + 1, REGS, REGS + 1])
def test_dense_lists_at_every_length_boundary(hip, n):
    """Full lists (cand_cap = n) of clusters of about five: the wave, the workgroup, both sort paths (cand_cap MAXK | MAXK + 1) and
    the fused boxes in registers | streamed (n REGS | REGS + 1).  skip_thr 0: every candidate with a score > 0 is walked."""
    classes, passes, lists = one_list(n, dense)
    res, h, mem = check(hip, classes, passes, lists, n, facts=False, skip_thr=0.0, conf="avg", expected=2)
    d, first, members, cluster_of, gap, cand = res[0]
    assert len(cand) == n and members.sum() == np.count_nonzero(cluster_of >= 0) == n
    assert n < WAVE or (np.any(members >= 2) and np.any(members == 1))


@pytest.mark.parametrize("n,lo,hi", [(110, WAVE, 2 * WAVE), (1800, THREADS, 2 * THREADS), (REGS, 2 * THREADS, REGS), (7000, REGS, 7000)])
def test_cluster_counts_across_the_wave_the_workgroup_and_the_register_limit(hip, n, lo, hi):
    """Lists of mostly singletons: the cluster count C passes lo on its way (a second wave takes part; a thread's second and third
    cluster; past REGS clusters, which only a streamed list can have) and ends below hi."""
    classes, passes, lists = one_list(n, sparse, seed=9)
    res, h, mem = check(hip, classes, passes, lists, n, facts=False, skip_thr=0.0, conf="max", expected=2)
    C = len(res[0][0])
    assert lo < C <= hi, C
    assert np.any(res[0][2] >= 2)


def test_5200_dense_candidates_stream_and_cross_the_second_cluster_of_a_thread(hip):
    n = 5200
    classes, passes, lists = one_list(n, dense, seed=37)
    res, h, mem = check(hip, classes, passes, lists, n, skip_thr=0.05, conf="avg", expected=2)
    assert len(res[0][0]) > THREADS


# ---- an overflowed list ---------------------------------------------------------------------------------------------------------------------------
def test_an_overflowed_list_reports_its_rows_and_leaves_its_slot_and_its_members_alone(hip):
    classes, passes, lists = gs.case("S4_two_passes")
    cap = 129                                    # image 0: 65 + 63 = 128 rows fit, image 1: 64 + 66 = 130 do not
    cand = gs.filled(hip, passes, classes, cap)
    assert [c[1] for c in cand.counts()] == [0, 0, 1, 1]
    pack = torch.full((hip.lib().mscnn_detections_multi_pack_bytes(4, 4 * cap),), 0xFF, dtype=torch.uint8, device="cuda")
    out, h, mem, per_seg = run_wbf(hip, cand, pack=pack, skip_thr=0.05, expected=2)
    want, wmem, res = expected_of(len(h), lists, cap, expected=2, thr=THR, skip_thr=0.05)
    assert res[2] is None and res[3] is None and out[2] == (None, None, 130) and out[3] == (None, None, 130) and per_seg[2] is None
    hdr = pack_views(h, 4, cap)[0]
    assert hdr[3].tolist() == [-1, 130, 2 * cap, 0] and hdr[4].tolist() == [-1, 130, 3 * cap, 0]
    table = 16 * 5
    assert guarded.all_poison(pack[table + 40 * 2 * cap:table + 40 * 4 * cap]), "rows of the overflowed lists"
    assert guarded.all_poison(pack[table + 40 * 4 * cap + 4 * 2 * cap:table + 44 * 4 * cap]), "tags of the overflowed lists"
    assert np.all(mem[2 * cap:] == -1), "members of the overflowed lists"
    assert np.array_equal(h, want) and np.array_equal(mem, wmem)


# ---- the buffer contract ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def arena(hip, monkeypatch):
    a = guarded.Arena("cuda")
    monkeypatch.setattr(hip, "torch", guarded.GuardedTorch(torch, a))
    yield a
    torch.cuda.synchronize()
    a.check()


@pytest.mark.parametrize("cap", [200, 4100])
def test_buffer_contract_of_the_wbf_merge(hip, arena, cap):
    """The candidate buffer, the workspace, the pack and the members buffer between guard bands (both paths: at 4100 slots image
    0's list is full, past REGS, and reads its fused boxes from the workspace): guards intact, the candidate buffer unwritten, of the
    pack and of members exactly the witness's bytes; unaligned bases and a short workspace are refused before any launch."""
    if cap == 200:
        classes, passes, lists = gs.case("S4_two_passes")
    else:
        classes = [2]
        passes = [Pass(0, [2050, 40], ncls=2, hw=BIG, seed=43, boxes=dense), Pass(1, [2050, 30], ncls=2, hw=BIG, seed=43, boxes=dense)]
        lists = gs.lists_of(passes, classes)
    S = len(lists)
    cand = gs.filled(hip, passes, classes, cap, arena)
    assert not arena.record(cand.buf).is_input
    nbytes = hip.lib().mscnn_detections_multi_pack_bytes(S, S * cap)
    wb = hip.lib().mscnn_detections_merge_wbf_workspace_bytes(S, cap)
    pack = arena.alloc(nbytes, torch.uint8)
    ws = arena.alloc(wb, torch.uint8)
    members = arena.alloc(S * cap, torch.int32)
    before = cand.buf.clone()
    out, h, mem, per_seg = run_wbf(hip, cand, pack=pack, ws=ws, members=members, skip_thr=0.05, expected=2)
    torch.cuda.synchronize()
    arena.check()
    assert torch.equal(cand.buf, before), "the op wrote the candidate buffer"
    want, wmem, res = expected_of(len(h), lists, cap, expected=2, thr=THR, skip_thr=0.05)
    assert facts_of(res, expected=2, thr=THR, skip_thr=0.05) == (True,) * 5 and (cap == 200 or len(res[0][5]) == 4100)
    assert np.array_equal(h, want), np.flatnonzero(h != want)[:8]
    assert np.array_equal(mem, wmem), np.flatnonzero(mem != wmem)[:8]
    # unaligned bases and a short workspace: refused, nothing written
    L, Cc = hip.lib(), hip.C
    ex = (Cc.c_int * S)(*([2] * S))
    wp = Cc.byref(hip.WbfParams(THR, 0.05, 1, 0))
    off = arena.offset_view(cand.buf, 8)
    pack2 = arena.alloc(nbytes + 16, torch.uint8)
    ws2 = arena.alloc(wb + 16, torch.uint8)
    mem2 = arena.alloc(S * cap * 4 + 16, torch.uint8)
    for c_, w_, p_, m_, what, al in ((off, ws2, pack2, mem2, "cand", 16), (cand.buf, ws2[8:], pack2, mem2, "workspace", 16),
                                     (cand.buf, ws2, pack2[8:], mem2, "pack_dev", 16), (cand.buf, ws2, pack2, mem2[2:], "members_dev", 4)):
        assert L.mscnn_detections_merge_wbf_fwd(wp, ex, S, hip._dev(c_), cap, hip._dev(p_), hip._dev(m_), hip._dev(w_), Cc.c_size_t(wb),
                                                hip._stream()) != 0
        assert f"detections_merge_wbf: {what} must be {al}-byte aligned" in L.mscnn_last_error().decode()
    assert L.mscnn_detections_merge_wbf_fwd(wp, ex, S, hip._dev(cand.buf), cap, hip._dev(pack2), hip._dev(mem2), hip._dev(ws2),
                                            Cc.c_size_t(wb - 1), hip._stream()) == 3      # MSCNN_ERR_WORKSPACE
    assert f"workspace {wb - 1} < {wb}" in L.mscnn_last_error().decode()
    torch.cuda.synchronize()
    assert guarded.all_poison(pack2) and guarded.all_poison(ws2) and guarded.all_poison(mem2) and torch.equal(cand.buf, before)


# ---- Net level ----------------------------------------------------------------------------------------------------------------------------------
def segs_of(classes, p):
    return [dict(cls_id=c, bbox_mean=(0, 0, 0, 0), bbox_std=STD, proposal_thr=-10.0, ratios=p["ratios"], org_hw=p["org_hw"], nms_overlap=0.5)
            for c in classes]


def flat(res):
    return b"".join(np.ascontiguousarray(a).tobytes() for img in res[0] for seg in img for a in seg) + repr(res[1]).encode()


def test_net_wbf_is_the_op_in_place_of_the_merge_with_its_members_and_off_again_the_merge_alone(hip):
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=96, width=320))
    synth.load_into(n, "mid")
    img = gs.frame_u8(375, 1242, 41)
    classes = [2, 3]

    def run(keep_blobs):
        """A frame and its mirror, merged with a plain _add each: (detect_merge_end's result, the forwards' blobs and params)."""
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

    assert n.get_wbf() is None
    never, _ = run(False)                                  # before the setting was ever touched
    with pytest.raises(mnet.NetError, match="did not run weighted boxes fusion"):
        n.detect_merge_members()
    n.set_wbf(THR, skip_thr=0.05, conf="avg", expected=0, max_out=50)
    assert n.get_wbf() == dict(thr=THR, skip_thr=0.05, conf="avg", expected=0, max_out=50)
    fused, fw = run(True)
    members = n.detect_merge_members()
    n.set_wbf(THR, skip_thr=0.05, conf="avg", expected=1, max_out=50)
    fused1, _ = run(False)
    n.set_wbf(None)
    plain, _ = run(False)
    with pytest.raises(mnet.NetError, match="did not run weighted boxes fusion"):
        n.detect_merge_members()
    assert flat(never) == flat(plain), "off again: what it always returned"
    # the same blobs through the ops: two plain adds are two views of the one frame, expected 0 -> 2
    cand = hip.Candidates(len(classes), gs.NET_CAP)
    for blobs, p, flipped in fw:
        cand.add(*[dev(b) for b in blobs], 1, segs_of(classes, p), views=[FLIP] if flipped else None)
    ref_plain = cand.merge()
    ref2, mem2 = cand.merge_wbf(THR, skip_thr=0.05, conf="avg", expected=2, max_out=50)
    ref1, _ = cand.merge_wbf(THR, skip_thr=0.05, conf="avg", expected=1, max_out=50)
    differs = scaled = 0
    for ci in range(len(classes)):
        for got, ref in ((plain, ref_plain), (fused, ref2), (fused1, ref1)):
            dets, pas, row = got[0][0][ci]
            assert same_bits(dets, ref[ci][0]) and np.array_equal((pas << 24) | row, ref[ci][1]) and got[1][0][ci] == ref[ci][2], ci
        assert np.array_equal(members[0][ci], mem2[ci]) and len(mem2[ci]) == len(fused[0][0][ci][0])
        differs += len(fused[0][0][ci][0]) != len(plain[0][0][ci][0]) or not same_bits(fused[0][0][ci][0], plain[0][0][ci][0])
        scaled += not same_bits(ref2[ci][0], ref1[ci][0])
    assert differs >= 1, "WBF returned the hard NMS's rows on this net: the case shows nothing"
    assert scaled >= 1, "expected 2 and expected 1 give the same rows: the views counted show nothing"


def test_net_expected_0_counts_the_views_of_each_frame_of_an_add_views(hip):
    """One batched forward of four images, list_of = [0, 0, 1, 0]: frame 0 has three views, frame 1 one."""
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=96, width=320, max_nms_num=200))
    synth.load_into(n, "mid")
    def small_u8(seed):      # a 120 x 400 frame: the seeded KITTI-shaped frame scaled down, as uint8 RGB
        x = synth.frame(120, 400, seed=seed)[0].transpose(1, 2, 0)[:, :, ::-1] + np.array([123.0, 117.0, 104.0])
        return np.ascontiguousarray(np.clip(np.round(x), 0, 255).astype(np.uint8))

    imgs = [small_u8(47), small_u8(48), small_u8(49), small_u8(47)]
    classes, list_of = [2, 3], [0, 0, 1, 0]
    K = len(classes)
    n.reshape_input("data", (4, 3, 96, 320))
    params = n.set_images("data", imgs)
    n.forward()
    R = n.blob_shape("proposals_score")[0]
    n.set_wbf(THR, skip_thr=0.05, conf="avg", expected=0)
    n.detect_merge_begin(2, K, R)
    n.detect_merge_add(params, classes, list_of=list_of)
    got = n.detect_merge_end()
    members = n.detect_merge_members()
    blobs = [dev(n.get_blob(b).reshape(R, -1)) for b in ("bbox_pred", "cls_pred", "proposals_score")]
    cand = hip.Candidates(2 * K, R)
    cand.add_views(*blobs, 4, [s for p in params for s in segs_of(classes, p)], list_of)
    ref, mem = cand.merge_wbf(THR, skip_thr=0.05, conf="avg", expected=[3] * K + [1] * K)
    ones, _ = cand.merge_wbf(THR, skip_thr=0.05, conf="avg", expected=1)
    total = 0
    for f in range(2):
        for ci in range(K):
            dets, pas, row = got[0][f][ci]
            s = f * K + ci
            assert same_bits(dets, ref[s][0]) and np.array_equal((pas << 24) | row, ref[s][1]) and got[1][f][ci] == ref[s][2], (f, ci)
            assert np.array_equal(members[f][ci], mem[s])
            total += len(dets)
    assert total > 3
    assert any(not same_bits(ref[s][0], ones[s][0]) for s in range(K)), "frame 0's three views mark nothing down: the case shows nothing"
    assert all(same_bits(ref[s][0], ones[s][0]) for s in range(K, 2 * K)), "frame 1 has one view: expected 1"
