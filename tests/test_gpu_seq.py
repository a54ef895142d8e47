"""Seq-NMS over the candidate lists of a clip's frames on the GPU: mscnn_detections_merge_seq_fwd through the HIP ABI on synthetic, seeded
clips (tests/seq_cases.py: one forward of T images = the T frames, built as tests/test_gpu_soft.py builds its passes), Net.set_seq_nms /
detect_merge_sequences on a reduced deploy, and the drivers' --seq-nms.  No pin on the reference, whose scripts run one forward per
image and look at no other frame: the check is tests/seq_witness.py.

The op is IEEE operations only and every maximum it takes is one under a total order, so the bar is bit equality, not a tolerance: the
whole pack -- header, table, rows, tags, and every byte the op must leave alone (the pack and the sequence buffer start as 0xFF poison)
-- is compared BYTE FOR BYTE with what the witness says the op writes, and so is the sequence buffer.

The two shipped clips first show ON THE WITNESS'S OWN RESULT the six facts of seq_witness.seq_facts: a case can not pass with a
per-frame NMS, without the rescoring, without the suppression, with paths that must span the clip, with a DP that is run once, or
with a first-match instead of the argmax over the predecessors.

Shapes, the smallest at which the kernels can go wrong -- the boundaries of det_seq.hip beside the constants they come from:
  WAVE = 64                 a wave's lanes: a link word, a live word, the ballot of the suppression (m_t 64 | 65)
  THREADS = kSeqThreads     1024: a thread is a box of the frame at hand, top_k's bound (m_t 1024; 1030 candidates cut by top_k 1024)
  MAXK = kMaxK              4032: the merge's one-pass sort | the tiled path's sort (cand_cap 4032 | 4033)
  SEGS = kSegsPerLaunch     32 segments per sort / enter launch (K = 33 chains x T = 2: 66 segments, three launches)
  kSeqLinkRows = 4          rows per workgroup of the link kernel (every m_t above that is no multiple of 4)
  kSeqMaxFrames = 256       num_frames' bound (refused above; the live masks of 256 frames are the kernel's 32 KB of LDS)"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import guarded                                   # noqa: E402
import seq_cases as sc                           # noqa: E402
import seq_witness as sq                         # noqa: E402
import test_gpu_soft as gs                       # noqa: E402  (Pass, dense, filled, pack_views, case)
from mscnn_amd import net as mnet, synth, zoo   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVE, THREADS, MAXK = 64, 1024, 4032
LINK = sc.LINK
Pass, dense, BIG, STD = gs.Pass, gs.dense, gs.BIG, gs.STD
same_bits, pack_views, dev = gs.same_bits, gs.pack_views, gs.dev


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X: torch.cuda.is_available() is False")
    from mscnn_amd import hipapi
    hipapi.lib()
    return hipapi


def poison(hip, S, cap):
    return (torch.full((hip.lib().mscnn_detections_multi_pack_bytes(S, S * cap),), 0xFF, dtype=torch.uint8, device="cuda"),
            torch.full((S * cap,), -1, dtype=torch.int32, device="cuda"))


def run_seq(hip, cand, T, pack=None, ws=None, seq=None, link_thr=LINK, **kw):
    """The op on a 0xFF-poisoned pack and sequence buffer: (merge_seq's segments, the pack's bytes, the sequence buffer's int32, the ids
    per segment)."""
    p, q = poison(hip, cand.S, cand.cap)
    pack = p if pack is None else pack
    seq = q if seq is None else seq
    (out, h), per = cand.merge_seq(link_thr, T, raw_pack=True, pack=pack, ws=ws, seq=seq, **kw)
    return out, h, seq.cpu().numpy(), per


def check(hip, classes, passes, lists, T, cap, facts=False, cand=None, **kw):
    """The op against the witness, byte for byte; kw: link_thr, nms_overlap, score_thr, top_k, rescore, max_out."""
    cand = gs.filled(hip, passes, classes, cap) if cand is None else cand
    out, h, got_seq, per = run_seq(hip, cand, T, **kw)
    want, wseq, res, traces = sc.expected_of(len(h), lists, T, cap, **kw)
    if facts:
        fkw = {k: v for k, v in kw.items() if k in ("link_thr", "nms_overlap", "score_thr", "top_k")}
        assert sc.facts_of(lists, T, cap=cap, **fkw) == (True,) * 6, "the case shows nothing: facts 1 .. 6"
    assert np.array_equal(h, want), np.flatnonzero(h != want)[:8]
    assert np.array_equal(got_seq, wseq), np.flatnonzero(got_seq != wseq)[:8]
    for (d, t, c), ids, r in zip(out, per, res):
        assert (r is None and d is None) or (same_bits(d, r[0]) and c == r[3] and np.array_equal(ids, r[4]))
    return res, traces, h, got_seq


# ---- the shipped clips, every parameter ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rescore", ["avg", "max"])
@pytest.mark.parametrize("score_thr", [0.05, 0.3])
@pytest.mark.parametrize("name", list(sc.CLIPS))
def test_the_pack_and_the_sequences_are_byte_equal_to_the_witness(hip, name, score_thr, rescore):
    classes, passes, lists, T = sc.clip(name)
    cap = 64
    cand = gs.filled(hip, passes, classes, cap)
    full = None
    for max_out in (0, 1, 7):
        res, traces, h, got_seq = check(hip, classes, passes, lists, T, cap, facts=(score_thr == 0.05 and max_out == 0), cand=cand,
                                        score_thr=score_thr, rescore=rescore, max_out=max_out)
        full = res if max_out == 0 else full
        if max_out == 1 or (max_out and score_thr == 0.05):      # (at score_thr 0.3 the short clip has no list of more than 7 rows)
            assert any(len(r[0]) > max_out for r in full), "max_out cuts no list: the case shows nothing"
        for r, fr in zip(res, full):      # max_out cuts the output, it changes no kept row and no sequence
            n = len(fr[0]) if max_out == 0 else min(max_out, len(fr[0]))
            assert len(r[0]) == n and same_bits(r[0], fr[0][:n]) and np.array_equal(r[4], fr[4][:n])
    entered, cands = sum(len(e[0]) for tr in traces for e in tr["ent"]), sum(r[3] for r in full)
    assert entered < cands and (score_thr == 0.05 or 2 * entered < cands), "score_thr cuts no list: the case shows nothing"
    if name == "T9_empty_4":
        tr = traces[0]
        assert len(tr["ent"][4][0]) == 0 and all(not (p[0][0] < 4 <= p[-1][0]) for p in tr["paths"]), "a path crossed the empty frame"
        assert pack_views(h, len(lists), cap)[0][1 + 4].tolist() == [0, 0, 4 * cap, 0]


def test_twice_into_the_same_pack_gives_the_same_bytes_and_a_null_seq_dev_the_same_pack(hip):
    classes, passes, lists, T = sc.clip("T8")
    cap = 64
    cand = gs.filled(hip, passes, classes, cap)
    pack, seq = poison(hip, cand.S, cap)
    ws = torch.full((hip.lib().mscnn_detections_merge_seq_workspace_bytes(T, len(classes), cap, 300),), 0xFF, dtype=torch.uint8, device="cuda")
    _, h1, s1, _ = run_seq(hip, cand, T, pack=pack, ws=ws, seq=seq, score_thr=0.05)
    _, h2, s2, _ = run_seq(hip, cand, T, pack=pack, ws=ws, seq=seq, score_thr=0.05)
    assert np.array_equal(h1, h2) and np.array_equal(s1, s2), "not idempotent"
    pack3, _ = poison(hip, cand.S, cap)
    (out, h3), none = cand.merge_seq(LINK, T, raw_pack=True, pack=pack3, seq=False, score_thr=0.05)
    assert none is None and np.array_equal(h1, h3)
    want, wseq, _, _ = sc.expected_of(len(h1), lists, T, cap, score_thr=0.05)
    assert np.array_equal(h1, want) and np.array_equal(s1, wseq)


def test_two_chains_with_a_different_nms_overlap_in_every_frame(hip):
    classes, passes, lists, T = sc.clip("T8")
    ov = [(0.2, 0.3, 0.45, 0.6, 0.75)[(3 * s + s // 2) % 5] for s in range(len(lists))]
    assert len(set(ov[0::2])) > 2 and ov[0::2] != ov[1::2]
    res, traces, _, _ = check(hip, classes, passes, lists, T, 64, score_thr=0.05, nms_overlap=ov)
    base = sc.expected_of(16 * (len(lists) + 1) + 44 * len(lists) * 64, lists, T, 64, score_thr=0.05)[2]
    assert any(len(a[0]) != len(b[0]) for a, b in zip(res, base)), "the overlaps change nothing: the case shows nothing"


# ---- the boundaries -------------------------------------------------------------------------------------------------------------------------------
_cache = {}


def dense_clip(T, n, seed=7, ncls=2, classes=(2,)):
    """(classes, passes, lists) of T frames of n candidates each in clusters of about five on the same grid in every frame."""
    key = (T, n, seed, ncls, tuple(classes))
    if key not in _cache:
        p = Pass(0, [n] * T, ncls=ncls, hw=BIG, seed=seed, boxes=dense)
        _cache[key] = (list(classes), [p], gs.lists_of([p], list(classes)))
    return _cache[key]


@pytest.mark.parametrize("T", [1, 2])
def test_one_frame_and_two(hip, T):
    classes, passes, lists, _ = sc.clip(T=T, classes=[2, 3], tracks=9, dup=2, lone=3, seed=5)
    res, traces, _, _ = check(hip, classes, passes, lists, T, 40, score_thr=0.05)
    assert all(len(p) <= T for tr in traces for p in tr["paths"]) and (T == 1 or any(len(p) == 2 for tr in traces for p in tr["paths"]))


@pytest.mark.parametrize("n,top_k", [(WAVE, 1024), (WAVE + 1, 1024), (THREADS, 1024), (THREADS + 6, 1024), (300, 64), (300, 65)])
def test_entered_boxes_at_the_wave_and_the_workgroup(hip, n, top_k):
    """Two frames of n candidates, score_thr 0: m_t = min(n, top_k) -- 64 | 65 (by the list and by top_k), 1024, and 1030 cut to 1024."""
    classes, passes, lists = dense_clip(2, n)
    res, traces, _, _ = check(hip, classes, passes, lists, 2, n, score_thr=0.0, top_k=top_k)
    assert [len(e[0]) for e in traces[0]["ent"]] == [min(n, top_k)] * 2
    assert any(len(p) == 2 for p in traces[0]["paths"]) and len(traces[0]["suppressed"]) > 0


@pytest.mark.parametrize("cap", [MAXK, MAXK + 1])
def test_both_sort_paths(hip, cap):
    """cand_cap 4032 | 4033: the one-pass sort against the tiled sort; the lists hold about 100 candidates, so the loop stays short."""
    classes, passes, lists = dense_clip(3, 100, seed=11, ncls=3, classes=(2, 3))
    res, traces, _, _ = check(hip, classes, passes, lists, 3, cap, score_thr=0.05)
    assert any(len(p) == 3 for tr in traces for p in tr["paths"])


def test_33_chains_of_two_frames_cross_the_launch_boundary(hip):
    classes = list(range(2, 35))
    classes_, passes, lists = dense_clip(2, 14, seed=13, ncls=34, classes=classes)
    assert len(lists) == 66
    res, traces, _, _ = check(hip, classes, passes, lists, 2, 20, score_thr=0.0)
    assert sum(len(p) == 2 for tr in traces for p in tr["paths"]) > 33


def test_a_score_threshold_cuts_a_list(hip):
    classes, passes, lists = dense_clip(2, 200, seed=17)
    res, traces, _, _ = check(hip, classes, passes, lists, 2, 200, score_thr=0.4)
    m = [len(e[0]) for e in traces[0]["ent"]]
    assert all(0 < v < 200 for v in m), m


def test_an_overflowed_middle_frame_is_an_empty_frame_and_its_rows_stay_untouched(hip):
    T, cap = 3, 40
    frames = sc.track_frames(T, tracks=9, dup=2, lone=2, seed=3, extra={1: cap + 5})
    p = sc.clip_pass(frames, seed=3)
    classes = [2]
    lists = gs.lists_of([p], classes)
    cand = gs.filled(hip, [p], classes, cap)
    assert [c[1] for c in cand.counts()] == [0, 1, 0]
    pack, seq = poison(hip, 3, cap)
    out, h, got_seq, per = run_seq(hip, cand, T, pack=pack, seq=seq, score_thr=0.05)
    want, wseq, res, traces = sc.expected_of(len(h), lists, T, cap, score_thr=0.05)
    assert res[1] is None and out[1] == (None, None, cap + 5) and per[1] is None
    assert pack_views(h, 3, cap)[0][2].tolist() == [-1, cap + 5, cap, 0]
    table = 16 * 4
    assert guarded.all_poison(pack[table + 40 * cap:table + 40 * 2 * cap]), "rows of the overflowed list"
    assert guarded.all_poison(pack[table + 40 * 3 * cap + 4 * cap:table + 40 * 3 * cap + 8 * cap]), "tags of the overflowed list"
    assert np.all(got_seq[cap:2 * cap] == -1), "sequence ids of the overflowed list"
    assert all(len(q) == 1 for q in traces[0]["paths"]), "a path crossed the overflowed frame"
    alone = sc.expected_of(len(h), [lists[0], [(np.zeros((0, 5)), np.zeros(0, np.int32))], lists[2]], T, cap, score_thr=0.05)[2]
    assert same_bits(res[0][0], alone[0][0]) and same_bits(res[2][0], alone[2][0]), "the neighbours behave as beside an empty frame"
    assert np.array_equal(h, want) and np.array_equal(got_seq, wseq)


def test_an_overflowed_list_on_the_tiled_sort_path_is_an_empty_frame_too(hip):
    """cand_cap 4033 (list after list through the tiled path's key kernel, whose count is 0 for an overflowed list): the middle frame
    wants 4040 rows in."""
    cap = MAXK + 1
    p = Pass(0, [60, cap + 7, 60], ncls=2, hw=BIG, seed=19, boxes=dense)
    lists = gs.lists_of([p], [2])
    cand = gs.filled(hip, [p], [2], cap)
    assert [c[1] for c in cand.counts()] == [0, 1, 0]
    out, h, got_seq, per = run_seq(hip, cand, 3, score_thr=0.05)
    want, wseq, res, traces = sc.expected_of(len(h), lists, 3, cap, score_thr=0.05)
    assert res[1] is None and out[1] == (None, None, cap + 7) and all(len(q) == 1 for q in traces[0]["paths"])
    assert len(res[0][0]) > 5 and len(res[2][0]) > 5
    assert np.array_equal(h, want), np.flatnonzero(h != want)[:8]
    assert np.array_equal(got_seq, wseq), np.flatnonzero(got_seq != wseq)[:8]


# ---- two identities against code that exists -------------------------------------------------------------------------------------------------------
def test_one_frame_is_the_hard_merge_byte_for_byte(hip):
    classes, passes, lists = gs.case("S4_two_passes")
    cap = 200
    cand = gs.filled(hip, passes, classes, cap)
    p0, _ = poison(hip, cand.S, cap)
    hard, h0 = cand.merge(raw_pack=True, pack=p0)
    p1, _ = poison(hip, cand.S, cap)
    (out, h1), _ = cand.merge_seq(LINK, 1, score_thr=0.0, top_k=1024, rescore="avg", raw_pack=True, pack=p1, seq=False)
    assert all(0 < len(d) < c for d, _, c in hard)
    assert np.array_equal(h0, h1), np.flatnonzero(h0 != h1)[:8]


def test_a_link_threshold_no_pair_exceeds_is_the_hard_merge_in_every_frame(hip):
    classes, passes, lists, T = sc.clip("T8")
    cap = 64
    cand = gs.filled(hip, passes, classes, cap)
    _, _, _, traces = sc.expected_of(16 * 17 + 44 * 16 * cap, lists, T, cap, link_thr=0.999, score_thr=0.0, top_k=1024)
    assert all(not l.any() for tr in traces for l in tr["links"][1:]), "a pair links on the witness"
    assert any(l.any() for tr in sc.expected_of(16 * 17 + 44 * 16 * cap, lists, T, cap, score_thr=0.0)[3] for l in tr["links"][1:])
    p0, _ = poison(hip, cand.S, cap)
    hard, h0 = cand.merge(raw_pack=True, pack=p0)
    p1, q1 = poison(hip, cand.S, cap)
    (out, h1), per = cand.merge_seq(0.999, T, score_thr=0.0, top_k=1024, raw_pack=True, pack=p1, seq=q1)
    assert np.array_equal(h0, h1), np.flatnonzero(h0 != h1)[:8]
    assert all(len(np.unique(ids)) == len(ids) for ids in per), "every box is a sequence of its own"


# ---- the buffer contract ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def arena(hip, monkeypatch):
    a = guarded.Arena("cuda")
    monkeypatch.setattr(hip, "torch", guarded.GuardedTorch(torch, a))
    yield a
    torch.cuda.synchronize()
    a.check()


@pytest.mark.parametrize("cap", [64, 4100])
def test_buffer_contract_of_the_seq_merge(hip, arena, cap):
    """The candidate buffer, the workspace, the pack and the sequence buffer between guard bands, on both sort paths: guards intact,
    the candidate buffer unwritten, of the pack and of the sequence buffer exactly the witness's bytes; every refusal -- unaligned
    bases, a short workspace, refused values -- leaves poison and guards intact."""
    classes, passes, lists, T = sc.clip("T8")
    S, K = len(lists), len(classes)
    cand = gs.filled(hip, passes, classes, cap, arena)
    assert not arena.record(cand.buf).is_input
    nbytes = hip.lib().mscnn_detections_multi_pack_bytes(S, S * cap)
    wb = hip.lib().mscnn_detections_merge_seq_workspace_bytes(T, K, cap, 300)
    pack = arena.alloc(nbytes, torch.uint8)
    ws = arena.alloc(wb, torch.uint8)
    seq = arena.alloc(S * cap, torch.int32)
    before = cand.buf.clone()
    out, h, got_seq, per = run_seq(hip, cand, T, pack=pack, ws=ws, seq=seq, score_thr=0.05)
    torch.cuda.synchronize()
    arena.check()
    assert torch.equal(cand.buf, before), "the op wrote the candidate buffer"
    want, wseq, res, _ = sc.expected_of(len(h), lists, T, cap, score_thr=0.05)
    assert np.array_equal(h, want), np.flatnonzero(h != want)[:8]
    assert np.array_equal(got_seq, wseq), np.flatnonzero(got_seq != wseq)[:8]
    # refusals: nothing written
    L, Cc = hip.lib(), hip.C
    ov = (Cc.c_double * S)(*([0.3] * S))
    good = dict(link_thr=LINK, score_thr=0.05, top_k=300, rescore=1, max_out=0)
    pack2 = arena.alloc(nbytes + 16, torch.uint8)
    ws2 = arena.alloc(wb + 16, torch.uint8)
    seq2 = arena.alloc(S * cap * 4 + 16, torch.uint8)

    def call(c_=cand.buf, w_=ws2, p_=pack2, q_=seq2, wbytes=wb, T_=T, K_=K, cap_=cap, ov_=ov, **kw):
        sp = hip.SeqNmsParams(*[dict(good, **kw)[k] for k in ("link_thr", "score_thr", "top_k", "rescore", "max_out")])
        return L.mscnn_detections_merge_seq_fwd(ov_, Cc.byref(sp), T_, K_, hip._dev(c_), cap_, hip._dev(p_), hip._dev(q_), hip._dev(w_),
                                                Cc.c_size_t(wbytes), hip._stream())

    off = arena.offset_view(cand.buf, 8)
    for kw, text in ((dict(c_=off), "cand must be 16-byte aligned"), (dict(w_=ws2[8:]), "workspace must be 16-byte aligned"),
                     (dict(p_=pack2[8:]), "pack_dev must be 16-byte aligned"), (dict(q_=seq2[2:]), "seq_dev must be 4-byte aligned"),
                     (dict(T_=257, K_=1), "num_frames 257 is outside [1, 256]"), (dict(T_=0), "num_frames 0 is outside"), (dict(K_=0), "num_slots 0"),
                     (dict(cap_=0), "cand_cap 0"), (dict(top_k=0), "top_k 0 is outside [1, 1024]"), (dict(top_k=1025), "top_k 1025 is outside"),
                     (dict(link_thr=0.0), "link_thr 0 is not inside (0, 1)"), (dict(link_thr=float("nan")), "link_thr nan"),
                     (dict(score_thr=-1.0), "score_thr -1 is not a finite value >= 0"), (dict(rescore=3), "rescore 3 is neither 1 (avg) nor 2 (max)"),
                     (dict(max_out=-1), "max_out -1")):
        assert call(**kw) == 1, kw      # MSCNN_ERR_BAD_ARG
        assert "detections_merge_seq: " + text in L.mscnn_last_error().decode(), (kw, L.mscnn_last_error().decode())
    bad = (Cc.c_double * S)(*([0.3] * (S - 1) + [float("nan")]))
    assert call(ov_=bad) == 1 and f"segment {S - 1}: nms_overlap is NaN" in L.mscnn_last_error().decode()
    assert call(wbytes=wb - 1) == 3 and f"workspace {wb - 1} < {wb}" in L.mscnn_last_error().decode()      # MSCNN_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert guarded.all_poison(pack2) and guarded.all_poison(ws2) and guarded.all_poison(seq2) and torch.equal(cand.buf, before)


# ---- Net level ----------------------------------------------------------------------------------------------------------------------------------
def segs_of(classes, p):
    return [dict(cls_id=c, bbox_mean=(0, 0, 0, 0), bbox_std=STD, proposal_thr=-10.0, ratios=p["ratios"], org_hw=p["org_hw"], nms_overlap=0.5)
            for c in classes]


def flat(res):
    return b"".join(np.ascontiguousarray(a).tobytes() for img in res[0] for seg in img for a in seg) + repr(res[1]).encode()


def small_u8(seed, shift=0):
    """A 120 x 400 frame: the seeded KITTI-shaped frame scaled down, as uint8 RGB, shifted `shift` pixels to the right."""
    x = synth.frame(120, 400, seed=seed)[0].transpose(1, 2, 0)[:, :, ::-1] + np.array([123.0, 117.0, 104.0])
    return np.ascontiguousarray(np.roll(np.clip(np.round(x), 0, 255).astype(np.uint8), shift, axis=1))


def clip_net(imgs):
    """The reduced deploy with a clip of len(imgs) frames forwarded as one batch: (net, params, R)."""
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=96, width=320, max_nms_num=200))
    synth.load_into(n, "mid")
    n.reshape_input("data", (len(imgs), 3, 96, 320))
    params = n.set_images("data", imgs)
    n.forward()
    return n, params, n.blob_shape("proposals_score")[0]


def test_net_seq_nms_is_the_op_with_its_sequences_the_vote_behind_it_and_off_again_the_merge_alone(hip):
    T, classes = 4, [2, 3]
    K = len(classes)
    n, params, R = clip_net([small_u8(47, 2 * t) for t in range(T)])

    def run():
        n.detect_merge_begin(T, K, R)
        n.detect_merge_add(params, classes)
        return n.detect_merge_end()

    assert n.get_seq_nms() is None
    never = run()                                          # before the setting was ever touched
    with pytest.raises(mnet.NetError, match="did not run Seq-NMS"):
        n.detect_merge_sequences()
    kw = dict(score_thr=0.05, top_k=300, rescore="avg", max_out=50)
    n.set_seq_nms(LINK, **kw)
    assert n.get_seq_nms() == dict(link_thr=LINK, **kw)
    got = run()
    seqs = n.detect_merge_sequences()
    with pytest.raises(mnet.NetError, match="no merge is open"):
        n.detect_merge_end()
    with pytest.raises(mnet.NetError, match="did not run Seq-NMS"):      # the last _end failed, before it enqueued anything
        n.detect_merge_sequences()
    n.set_box_voting(0.5)
    voted = run()
    n.set_box_voting(None)
    # more than 256 frames: refused at _begin while the setting is on (nothing is opened), at _end when it was turned on behind _begin
    with pytest.raises(mnet.NetError, match=r"detect_merge_begin: num_frames 257 is outside \[1, 256\] while Seq-NMS is on \(set_seq_nms link_thr 0.5\)"):
        n.detect_merge_begin(257, K, 4)
    assert flat(run()) == flat(got), "the refused _begin opened nothing and changed nothing"
    n.set_seq_nms(None)
    n.detect_merge_begin(257, K, 4)
    n.set_seq_nms(LINK, **kw)
    with pytest.raises(mnet.NetError, match=r"detect_merge_end: num_frames 257 is outside \[1, 256\] while Seq-NMS is on"):
        n.detect_merge_end()
    n.set_seq_nms(None)
    plain = run()
    with pytest.raises(mnet.NetError, match="did not run Seq-NMS"):
        n.detect_merge_sequences()
    assert flat(never) == flat(plain), "off again: what it always returned"
    # the same blobs through the ops
    blobs = [dev(n.get_blob(b).reshape(R, -1)) for b in ("bbox_pred", "cls_pred", "proposals_score")]
    cand = hip.Candidates(T * K, R)
    cand.add(*blobs, T, [s for p in params for s in segs_of(classes, p)])
    ref_plain = cand.merge()
    ref, ids = cand.merge_seq(LINK, T, **kw)
    ref_voted, _ = cand.merge_seq(LINK, T, vote_thr=0.5, **kw)
    differs = moved = linked = 0
    for t in range(T):
        for ci in range(K):
            s = t * K + ci
            for res, want in ((plain, ref_plain), (got, ref), (voted, ref_voted)):
                dets, pas, row = res[0][t][ci]
                assert same_bits(dets, want[s][0]) and np.array_equal((pas << 24) | row, want[s][1]) and res[1][t][ci] == want[s][2], (t, ci)
            assert np.array_equal(seqs[t][ci], ids[s]) and len(ids[s]) == len(got[0][t][ci][0])
            differs += len(got[0][t][ci][0]) != len(plain[0][t][ci][0]) or not same_bits(got[0][t][ci][0], plain[0][t][ci][0])
            moved += not same_bits(voted[0][t][ci][0], got[0][t][ci][0])
    for ci in range(K):
        linked += len(set(ids[ci].tolist()) & set(ids[K + ci].tolist())) > 0
    assert differs >= 1, "Seq-NMS returned the hard NMS's rows on this net: the case shows nothing"
    assert linked >= 1, "no sequence spans two frames on this net: the case shows nothing"
    assert moved >= 1, "the vote behind Seq-NMS moved no box: the case shows nothing"


def test_net_the_same_frame_fed_four_times_keeps_the_hard_merges_boxes_and_every_sequence_has_four_members(hip):
    """One forward of one frame, its rows added to the lists of four frames (list_of = [t]): identical lists.  The best path is the best
    live box in every frame (scores distinct: no other path reaches T times the best score), it suppresses in every frame what the hard
    NMS's pick suppresses, and so on down the list.  T s is exact in double for a float s and T = 4, so avg gives s back."""
    T, classes = 4, [2]
    n, params, R = clip_net([small_u8(47)])
    blobs = [dev(n.get_blob(b).reshape(R, -1)) for b in ("bbox_pred", "cls_pred", "proposals_score")]
    cap = T * R
    cand = hip.Candidates(T, cap)
    for t in range(T):
        cand.add_views(*blobs, 1, segs_of(classes, params[0]), [t])
    lists = []
    o0 = (8 * T + 255) // 256 * 256
    o1 = o0 + (32 * T * cap + 255) // 256 * 256
    for t, (wanted, over) in enumerate(cand.counts()):
        box = cand.buf[o0 + 32 * t * cap:o0 + 32 * (t * cap + wanted)].cpu().numpy().view(np.float64).reshape(wanted, 4)
        prob = cand.buf[o1 + 4 * t * cap:o1 + 4 * (t * cap + wanted)].cpu().numpy().view(np.float32)
        lists.append(np.concatenate([box, prob[:, None].astype(np.float64)], 1))
        assert not over and wanted > 5
    assert all(np.array_equal(l, lists[0]) for l in lists)
    assert len(np.unique(lists[0][:, 4])) == len(lists[0]), "two candidates share a score: the witness's premise"
    rows, tr = sq.seq_nms(lists, LINK, [0.5] * T, 0.0, 1024)
    assert all(len(p) == T and len({j for _, j in p}) == 1 for p in tr["paths"]), "the witness itself leaves a box's own column"
    n.set_seq_nms(LINK, score_thr=0.0, top_k=1024)
    n.detect_merge_begin(T, 1, cap)
    for t in range(T):
        n.detect_merge_add(params, classes, list_of=[t])
    got = n.detect_merge_end()
    seqs = n.detect_merge_sequences()
    hard = cand.merge()
    for t in range(T):
        dets, pas, row = got[0][t][0]
        assert len(dets) > 3 and same_bits(dets, hard[t][0]) and np.array_equal((pas << 24) | row, hard[t][1]) and np.all(pas == t), t
        assert np.array_equal(seqs[t][0], seqs[0][0]) and len(set(seqs[t][0].tolist())) == len(dets), "every sequence has T members"


# ---- the drivers ----------------------------------------------------------------------------------------------------------------------------------
def run_driver(tool, tmp_path, tag, *args):
    out = tmp_path / tag
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--out", str(out), "--comp-id", "t", *args], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return {f: (out / f).read_bytes() for f in sorted(os.listdir(out))}, r.stdout


def parsed(data, cols):
    rows = [[float(v) for v in line.split(",")] for line in data.decode().splitlines() if line.strip()]
    assert all(len(r) == cols for r in rows)
    return np.array(rows, np.float64).reshape(-1, cols)


@pytest.mark.parametrize("tool,common,stem", [
    ("run_mscnn_detection.py", ["--synthetic", "4", "--cls-ids", "2"], "t_car"),
    ("run_cascademscnn.py", ["--model", "kitti_car/cascade-mscnn-7s-576-2x", "--input-size", "192,448", "--max-nms-num", "150", "--synthetic", "4"], None)])
def test_driver_seq_nms_over_clips_of_three_writes_results_and_tubelets(hip, tmp_path, tool, common, stem):
    """Four synthetic frames, --clip 3 --batch 3: a clip of three frames (one forward) and a last clip of one.  The result files parse
    and keep their format; the tubelet files hold the same rows with a sequence column; a sequence id is unique within a clip, class
    and frame."""
    if tool == "run_mscnn_detection.py":
        deploy = tmp_path / "deploy.prototxt"
        deploy.write_text(zoo.prototxt("kitti_car/mscnn-7s-576", height=96, width=320))
        common = ["--prototxt", str(deploy)] + common
    tubes = tmp_path / "tubes"
    files, _ = run_driver(tool, tmp_path, "seq", *common, "--seq-nms", "--clip", "3", "--batch", "3", "--soft-thr", "0.05", "--tubelets-out", str(tubes))
    assert len(files) == 1 and (stem is None or list(files) == [stem + ".txt"])
    name = list(files)[0]
    dets = parsed(files[name], 6)
    tube_name = name.replace("_results", "")
    assert sorted(os.listdir(tubes)) == [tube_name]
    tub = parsed((tubes / tube_name).read_bytes(), 7)
    assert len(dets) > 4 and np.array_equal(tub[:, [0, 2, 3, 4, 5, 6]], dets) and set(dets[:, 0].astype(int)) <= {1, 2, 3, 4}
    assert np.all(tub[:, 1] >= 0) and np.all(tub[:, 1] == np.floor(tub[:, 1]))
    for img in np.unique(tub[:, 0]):
        ids = tub[tub[:, 0] == img, 1]
        assert len(np.unique(ids)) == len(ids), "a sequence has one box per frame"


def test_the_drivers_default_path_opens_no_merge_and_never_touches_the_setting(hip, tmp_path, monkeypatch, capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("run_mscnn_detection", os.path.join(ROOT, "tools", "run_mscnn_detection.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    deploy = tmp_path / "deploy.prototxt"
    deploy.write_text(zoo.prototxt("kitti_car/mscnn-7s-576", height=96, width=320))

    def forbidden(self, *a, **k):
        raise AssertionError("the default path reached the merge / Seq-NMS code")

    for name in ("set_seq_nms", "detect_merge_begin", "detect_merge_sequences"):
        monkeypatch.setattr(mnet.Net, name, forbidden)
    for extra in ([], ["--batch", "2"]):
        assert drv.main(["--prototxt", str(deploy), "--synthetic", "2", "--out", str(tmp_path / ("o" + str(len(extra)))), "--comp-id", "t", "--cls-ids", "2",
                         *extra]) == 0
    capsys.readouterr()


PLAIN = ["--synthetic", "3", "--cls-ids", "2"]
CASCADE = ["--model", "kitti_car/cascade-mscnn-7s-576-2x", "--input-size", "192,448", "--max-nms-num", "150", "--synthetic", "3"]


@pytest.mark.parametrize("tool,common,fixture", [("run_mscnn_detection.py", PLAIN, "plain_b1"), ("run_mscnn_detection.py", PLAIN + ["--batch", "2"], "plain_b2"),
                                                 ("run_cascademscnn.py", CASCADE, "cascade_b1"), ("run_cascademscnn.py", CASCADE + ["--batch", "2"], "cascade_b2")])
def test_drivers_without_the_new_flags_write_the_parent_commits_files_byte_for_byte(hip, tmp_path, tool, common, fixture):
    """tests/golden/seq_drivers/*.txt: what the commit before Seq-NMS wrote for these very runs on an MI355X (three synthetic frames,
    the reduced deploys, seeded weights; recorded twice there, the two recordings equal).  The forward is not this change's business
    and is not edited by it: a difference here is the drivers' default path."""
    if tool == "run_mscnn_detection.py":
        deploy = tmp_path / "deploy.prototxt"
        deploy.write_text(zoo.prototxt("kitti_car/mscnn-7s-576", height=96, width=320))
        common = ["--prototxt", str(deploy)] + common
    files, _ = run_driver(tool, tmp_path, "plain", *common)
    assert len(files) == 1
    want = open(os.path.join(ROOT, "tests", "golden", "seq_drivers", fixture + ".txt"), "rb").read()
    assert len(want) > 1000 and list(files.values())[0] == want
