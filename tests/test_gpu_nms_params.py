"""bbNms's knobs on the final stage, on the GPU: type 'maxg' / 'max', ovrDnm 'union' / 'min', bbNms's thr and the plain stage's
det_thr, through the HIP ABI on synthetic ROI blobs (ncls = 2) and through the Net.

How every expectation is made: the existing default stage with nms_overlap = +inf suppresses nothing, so it returns every surviving
row, sorted, with its id (that path is pinned bit-exact elsewhere).  The numpy witness of nmsMax (tests/nms_witness.py) on exactly
those rows gives the keep set; a mode's detections must be those rows, bit for bit, and its ids those ids."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import nms_witness as wit                        # noqa: E402
from mscnn_amd import net as mnet, synth, zoo   # noqa: E402

INF = float("inf")
COMBOS = [(t, d) for t in wit.TYPES for d in wit.OVR_DNMS]
BIG = (10000, 10000)      # an original image no test box reaches: nothing is clipped


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


def plain_blobs(xywh, logit, image=None, score=None):
    """ROI blobs of the plain stage (ncls = 2) whose transformed boxes are the given integer [x y w h] (zero regression, ratio 1:
    ctr - w / 2 is exact on integers) and whose class-2 probability is sigmoid(logit), class-1 its complement.  score: the proposal
    score (default 0; under -10 the row is filtered out)."""
    xywh = np.asarray(xywh, np.float32).reshape(-1, 4)
    R = len(xywh)
    props = np.zeros((R, 6), np.float32)
    props[:, 0] = 0 if image is None else image
    props[:, 1:3] = xywh[:, :2]
    props[:, 3:5] = xywh[:, :2] + xywh[:, 2:]
    props[:, 5] = 0 if score is None else score
    cls_pred = np.zeros((R, 2), np.float32)
    cls_pred[:, 1] = logit
    return np.zeros((R, 8), np.float32), cls_pred, props


def seg_kw(cls_id=2, org_hw=BIG, nms_overlap=0.5):
    return dict(cls_id=cls_id, bbox_mean=(0, 0, 0, 0), bbox_std=(0.1, 0.1, 0.2, 0.2), proposal_thr=-10.0, ratios=(1.0, 1.0), org_hw=org_hw,
                nms_overlap=nms_overlap)


def all_rows(hip, blobs, **kw):
    """Every surviving row, sorted, and its id: the existing entry point with nms_overlap = +inf."""
    rows, ids = hip.detections(*[dev(b) for b in blobs], **dict(kw, nms_overlap=INF))
    return rows.cpu().numpy(), ids.cpu().numpy()


def check_modes(hip, blobs, overlap=0.5, **kw):
    """All four (type, ovr_dnm) combinations through the single-list and the one-pass entry points against the witness on the
    device's own rows.  Returns (rows, ids, {combo: keep mask})."""
    kw = dict(seg_kw(), **kw)
    kw["nms_overlap"] = overlap
    rows, ids = all_rows(hip, blobs, **kw)
    keeps = wit.keep_sets(rows, overlap)
    d = [dev(b) for b in blobs]
    for (t, dn), keep in keeps.items():
        nms = dict(type=t, ovr_dnm=dn)
        dets, got = hip.detections(*d, nms=nms, **kw)
        assert np.array_equal(got.cpu().numpy(), ids[keep]), (t, dn, got.cpu().numpy().tolist(), ids[keep].tolist())
        assert same_bits(dets.cpu().numpy(), rows[keep]), (t, dn)
        (mdets, mids, row0, nrows), = hip.detections_multi(*d, 1, [kw], nms=nms)
        assert (row0, nrows) == (0, len(blobs[2]))
        assert np.array_equal(mids, ids[keep]) and same_bits(mdets, rows[keep]), (t, dn)
    return rows, ids, keeps


# ---- separating cases ----------------------------------------------------------------------------------------------------------------
def test_chain_separates_greedy_from_non_greedy(hip):
    """A overlaps B, B overlaps C (6 / 14 each), A does not overlap C enough (2 / 18): 'maxg' keeps {A, C} -- B, suppressed, suppresses
    nothing -- 'max' keeps {A}."""
    blobs = plain_blobs([[100, 100, 10, 10], [104, 100, 10, 10], [108, 100, 10, 10]], [3.0, 2.0, 1.0])
    rows, ids, keeps = check_modes(hip, blobs, overlap=0.4)
    assert ids.tolist() == [0, 1, 2] and np.array_equal(rows[:, :4], [[100, 100, 10, 10], [104, 100, 10, 10], [108, 100, 10, 10]])
    assert keeps[("maxg", "union")].tolist() == [True, False, True]
    assert keeps[("max", "union")].tolist() == [True, False, False]


def test_nested_box_separates_union_from_min(hip):
    """A small box inside a large one: 36 / 400 of the union (kept), 36 / 36 of the smaller area (suppressed)."""
    blobs = plain_blobs([[50, 50, 20, 20], [55, 55, 6, 6]], [2.0, 1.0])
    _, ids, keeps = check_modes(hip, blobs)
    assert ids.tolist() == [0, 1]
    for t in wit.TYPES:
        assert keeps[(t, "union")].tolist() == [True, True] and keeps[(t, "min")].tolist() == [True, False]


def test_equal_scores_are_ordered_by_the_lower_row(hip):
    """Three overlapping boxes with one score: the lower row comes first in every mode, as in the default stage; the survivor is
    row 0, and with a filtered row in front of them still the lowest surviving row."""
    blobs = plain_blobs([[10, 10, 20, 20], [11, 10, 20, 20], [12, 10, 20, 20], [300, 300, 20, 20]], [1.5, 1.5, 1.5, 1.5])
    rows, ids, keeps = check_modes(hip, blobs)
    assert ids.tolist() == [0, 1, 2, 3] and len(set(rows[:, 4])) == 1
    for c in COMBOS:
        assert keeps[c].tolist() == [True, False, False, True]
    blobs = plain_blobs([[0, 0, 5, 5], [10, 10, 20, 20], [11, 10, 20, 20], [12, 10, 20, 20]], [1.5] * 4, score=[-11, 0, 0, 0])
    _, ids, keeps = check_modes(hip, blobs)
    assert ids.tolist() == [1, 2, 3] and all(keeps[c].tolist() == [True, False, False] for c in COMBOS)


def test_zero_area_and_negative_width_boxes_take_part_in_nothing(hip):
    """Clipping to a 100-wide image turns a box at x = 100 into width 0 and one at x = 105 into width -5 (run_mscnn_detection.m:
    tw = min(tw, orgW - tx)).  They lie on top of normal boxes and of each other, score highest and lowest: never suppressed,
    never suppressing, in every mode."""
    xywh = [[100, 10, 10, 30], [105, 10, 10, 30], [80, 10, 20, 30], [82, 10, 18, 30], [100, 12, 10, 30], [105, 12, 10, 30]]
    blobs = plain_blobs(xywh, [4.0, 3.5, 3.0, 2.0, 1.0, 0.5])
    rows, ids, keeps = check_modes(hip, blobs, org_hw=(1000, 100))
    assert ids.tolist() == [0, 1, 2, 3, 4, 5]
    assert rows[:, 2].tolist() == [0, -5, 20, 18, 0, -5]
    for c in COMBOS:
        assert keeps[c].tolist() == [True, True, True, False, True, True]


# ---- block seams ---------------------------------------------------------------------------------------------------------------------
def seam_blobs(n, seed):
    """n surviving rows in about n / 5 well-separated clusters of boxes of mixed sizes (so that the two denominators disagree) whose
    scores are spread over the whole ranking (so that a box and what it suppresses sit in different 64-column words, and chains
    A-B-C form), a few exact score ties, and filtered rows in between (ids differ from positions)."""
    rng = np.random.default_rng(seed)
    k = max(1, n // 5)
    member = rng.integers(0, k, n)
    centre = np.stack([300 * (member % 16) + 50, 300 * (member // 16) + 50], 1)
    xy = centre + rng.integers(-10, 11, (n, 2))
    wh = rng.choice([14, 20, 32, 48], (n, 2))
    logit = rng.permutation(np.linspace(-3.0, 3.0, n)) if n > 1 else np.array([0.5])
    if n > 8:
        logit[5] = logit[2]; logit[n - 1] = logit[n // 2]
        lo, hi = int(np.argmin(logit)), int(np.argmax(logit))      # the last box of the ranking lies on the first one: suppressed in
        xy[lo] = xy[hi] + 1; wh[lo] = wh[hi]                        # every mode, from the first word (n = 65: the only box of word 1)
    extra = n // 7 + 1
    at = np.sort(rng.choice(n + extra, extra, replace=False))
    xywh = np.zeros((n + extra, 4)); lg = np.zeros(n + extra); score = np.zeros(n + extra)
    live = np.setdiff1d(np.arange(n + extra), at)
    xywh[live] = np.concatenate([xy, wh], 1); lg[live] = logit
    xywh[at] = [60, 60, 40, 40]; score[at] = -11.0
    return plain_blobs(xywh, lg, score=score), live


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 257])
def test_block_seams_in_every_mode(hip, n):
    blobs, live = seam_blobs(n, 100 + n)
    rows, ids, keeps = check_modes(hip, blobs)
    assert len(rows) == n and sorted(ids.tolist()) == live.tolist()
    if n == 1:      # (a single box has one possible keep set)
        assert all(k.tolist() == [True] for k in keeps.values())
        return
    # the inputs separate the modes: at least three distinct keep sets among the four combinations
    assert len({k.tobytes() for k in keeps.values()}) >= 3, {c: int(k.sum()) for c, k in keeps.items()}
    assert all(0 < k.sum() < n for k in keeps.values())
    if n > 64:      # suppression crosses a 64-column word boundary: some suppressed box has every one of its suppressors in an earlier word
        for dn in wit.OVR_DNMS:
            over = wit.overlaps(rows, dn) > 0.5
            j = np.flatnonzero(over.any(0))
            last = np.array([np.flatnonzero(over[:, c]).max() for c in j])
            assert np.any(last // 64 < j // 64), dn


# ---- segments ------------------------------------------------------------------------------------------------------------------------
def two_image_blobs(order):
    """Two images: one of exactly 64 rows (clustered, as the seam inputs), one of 37 rows none of which survives the proposal
    filter; `order` says which comes first."""
    (b64, c64, p64), _ = seam_blobs(55, 7)                  # 55 surviving + 8 filtered = 63 rows ...
    b64 = np.concatenate([b64, b64[:1]]); c64 = np.concatenate([c64, c64[:1]]); p64 = np.concatenate([p64, p64[:1]])      # ... + 1 = 64
    assert len(p64) == 64
    rng = np.random.default_rng(3)
    b0, c0, p0 = plain_blobs(np.concatenate([rng.integers(0, 500, (37, 2)), rng.integers(10, 60, (37, 2))], 1), rng.normal(0, 1, 37),
                             score=np.full(37, -11.0))
    parts = [(b64, c64, p64), (b0, c0, p0)] if order == 0 else [(b0, c0, p0), (b64, c64, p64)]
    for i, (_, _, p) in enumerate(parts):
        p[:, 0] = i
    return tuple(np.concatenate([q[k] for q in parts]) for k in range(3)), [len(q[2]) for q in parts]


@pytest.mark.parametrize("order", [0, 1])
def test_segments_equal_the_per_range_stage_and_the_default_struct_the_existing_call(hip, order):
    blobs, counts = two_image_blobs(order)
    d = [dev(b) for b in blobs]
    segs = [seg_kw(cls_id=c) for _ in range(2) for c in (1, 2)]
    start = [0, counts[0]]
    surviving = []
    for t, dn in COMBOS:
        nms = dict(type=t, ovr_dnm=dn)
        out = hip.detections_multi(*d, 2, segs, max_rows_per_image=64, nms=nms)
        for s, (dets, ids, row0, rows) in enumerate(out):
            i = s // 2
            assert (row0, rows) == (start[i], counts[i]), s
            sl = slice(row0, row0 + rows)
            part = tuple(b[sl] for b in blobs)
            d1, i1 = hip.detections(*[dev(b) for b in part], nms=nms, **segs[s])      # the per-range stage: bit for bit
            assert np.array_equal(ids, i1.cpu().numpy()) and same_bits(dets, d1.cpu().numpy()), (t, dn, s)
            allr, alli = all_rows(hip, part, **segs[s])                                   # ... and the witness on the range's rows
            keep = wit.nms_max(allr, 0.5, greedy=(t == "maxg"), ovr_dnm=dn)
            assert np.array_equal(ids, alli[keep]) and same_bits(dets, allr[keep]), (t, dn, s)
            surviving.append(len(allr))
    assert sorted(set(surviving)) == [0, int((blobs[2][:, 5] >= -10).sum())] and max(surviving) >= 55      # one image has no surviving row
    # NULL and the default struct: the pack of the existing call, word for word
    _, old = hip.detections_multi(*d, 2, segs, max_rows_per_image=64, raw_pack=True)
    for nms in (hip.NMS_NULL, hip.NmsParams(0, 0, -INF, 0.0), dict()):
        _, new = hip.detections_multi(*d, 2, segs, max_rows_per_image=64, nms=nms, raw_pack=True)
        assert np.array_equal(old.view(np.uint32), new.view(np.uint32))
    assert sum(int(old.view(np.int32)[4 * (1 + s)]) for s in range(4)) > 0      # (the packs compared hold detections)


def cascade_blobs(rows_per_image, seed):
    """One cascade output (ncls = 2): decoded boxes [img x1 y1 x2 y2], probabilities, proposals; clustered as the seam inputs, one
    proposal of zero width (dropped)."""
    rng = np.random.default_rng(seed)
    parts = []
    for i, n in enumerate(rows_per_image):
        k = max(1, n // 5)
        member = rng.integers(0, k, n)
        xy = np.stack([300 * (member % 16) + 50, 300 * (member // 16) + 50], 1) + rng.integers(-10, 11, (n, 2))
        wh = rng.choice([14, 20, 32, 48], (n, 2))
        parts.append(np.concatenate([np.full((n, 1), i), xy, xy + wh - 1], 1).astype(np.float32))
    boxes = np.concatenate(parts)
    R = len(boxes)
    props = boxes.copy()
    props[3, 3] = props[3, 1] - 1                      # cw = x2 - x1 + 1 = 0
    p2 = rng.permutation(np.linspace(0.02, 0.98, R)).astype(np.float32)
    prob = np.stack([1 - p2, p2], 1).astype(np.float32)
    return boxes, prob, props


def test_cascade_segments_with_det_thr_thr_and_type_max(hip):
    """One cascade source, 2 images (64 and 41 rows) x 2 classes: det_thr > 0 (>=, on a row's exact probability) combined with bbNms's
    thr (strict, on another row's exact probability) and type 'max', both denominators; every segment against the per-range call and
    against the witness on the rows that pass both thresholds."""
    counts = [64, 41]
    boxes, prob, props = cascade_blobs(counts, 17)
    outs = [(dev(boxes), dev(prob), dev(props))]
    kw = [dict(cls_id=c, ratios=(1.0, 1.0), org_hw=BIG, nms_overlap=0.5) for _ in range(2) for c in (1, 2)]
    everything = hip.detections_cascade_multi(outs, 2, [dict(k, nms_overlap=INF) for k in kw], max_rows_per_image=64)
    # two probabilities that occur in segment 1, the higher one on a row that 'max' keeps under both denominators (whether a row is
    # kept depends on the rows before it only): where the threshold sits exactly on it, strict and non-strict differ visibly
    allr1, alli1 = everything[1][0], everything[1][1]
    n1 = len(allr1)
    assert n1 == 63                                    # image 0, class 2: 64 rows, one proposal of zero width
    kept = wit.nms_max(allr1, 0.5, False, "union") & wit.nms_max(allr1, 0.5, False, "min")
    k1 = int(np.flatnonzero(kept & (np.arange(n1) >= 35))[0])
    k2 = k1 + 8
    assert k2 < n1
    p_hi, p_lo = float(allr1[k1, 4]), float(allr1[k2, 4])
    assert p_hi > p_lo > 0 and float(np.float32(p_hi)) == p_hi
    _, old = hip.detections_cascade_multi(outs, 2, kw, det_thr=p_lo, max_rows_per_image=64, raw_pack=True)
    for nms in (hip.NMS_NULL, hip.NmsParams(0, 0, -INF, 0.0)):
        _, new = hip.detections_cascade_multi(outs, 2, kw, det_thr=p_lo, max_rows_per_image=64, nms=nms, raw_pack=True)
        assert np.array_equal(old.view(np.uint32), new.view(np.uint32))
    differs = False
    for dn in wit.OVR_DNMS:
        # thr on the higher probability: that row goes (strict >); det_thr on it: that row stays (>=)
        for thr, det_thr, k1_stays in ((p_hi, p_lo, False), (p_lo, p_hi, True)):
            nms = dict(type="max", ovr_dnm=dn, thr=thr)
            out = hip.detections_cascade_multi(outs, 2, kw, det_thr=det_thr, max_rows_per_image=64, nms=nms)
            start = [0, 64]
            for s, (dets, ids, row0, rows) in enumerate(out):
                i = s // 2
                assert (row0, rows) == (start[i], counts[i])
                sl = slice(row0, row0 + rows)
                d1, i1 = hip.detections_cascade(dev(boxes[sl]), dev(prob[sl]), dev(props[sl]), det_thr=det_thr, nms=nms, **kw[s])
                assert np.array_equal(ids, i1.cpu().numpy()) and same_bits(dets, d1.cpu().numpy()), (dn, s)
                allr, alli = everything[s][0], everything[s][1]
                passed = (allr[:, 4].astype(np.float32) >= np.float32(det_thr)) & (allr[:, 4] > thr)
                allr, alli = allr[passed], alli[passed]
                keep = wit.nms_max(allr, 0.5, greedy=False, ovr_dnm=dn)
                assert np.array_equal(ids, alli[keep]) and same_bits(dets, allr[keep]), (dn, s)
                if s == 1:
                    assert (alli1[k1] in ids) == k1_stays and passed.sum() == k1 + int(k1_stays)
                differs = differs or keep.tobytes() != wit.nms_max(allr, 0.5, greedy=True, ovr_dnm=dn).tobytes()
    assert differs      # type 'max' is not 'maxg' on these inputs


# ---- thr and the plain stage's det_thr -----------------------------------------------------------------------------------------------
def test_thr_is_strict_det_thr_is_not_and_det_thr_commutes_with_the_greedy_nms(hip):
    blobs, _ = seam_blobs(129, 41)
    d = [dev(b) for b in blobs]
    kw = seg_kw()
    rows, ids = all_rows(hip, blobs, **kw)
    dflt, dflt_ids = hip.detections(*d, **kw)
    dflt, dflt_ids = dflt.cpu().numpy(), dflt_ids.cpu().numpy()
    # a probability that occurs (a float's value, exact in both types), on a row that both types keep when it passes the threshold
    # (whether a row is kept depends on the rows before it only), with distinct neighbours
    cand = np.flatnonzero(wit.nms_max(rows, 0.5, greedy=False) & (np.arange(len(rows)) >= 40))
    K = int([k for k in cand if rows[k - 1, 4] > rows[k, 4] > rows[k + 1, 4]][0])
    t = rows[K, 4]
    assert K + 30 < len(rows)

    def run(**nms):
        a, b = hip.detections(*d, nms=nms, **kw)
        (ma, mb, _, _), = hip.detections_multi(*d, 1, [kw], nms=nms)
        assert same_bits(a.cpu().numpy(), ma) and np.array_equal(b.cpu().numpy(), mb)
        return ma, mb

    # bbNms's thr: prob > thr -- the row at exactly thr goes
    for tp in wit.TYPES:
        dets, got = run(type=tp, thr=float(t))
        keep = wit.nms_max(rows[:K], 0.5, greedy=(tp == "maxg"))
        assert np.array_equal(got, ids[:K][keep]) and same_bits(dets, rows[:K][keep]) and ids[K] not in got
        # det_thr: prob >= det_thr -- the row at exactly det_thr stays
        dets, got = run(type=tp, det_thr=float(t))
        keep = wit.nms_max(rows[:K + 1], 0.5, greedy=(tp == "maxg"))
        assert np.array_equal(got, ids[:K + 1][keep]) and same_bits(dets, rows[:K + 1][keep]) and ids[K] in got
    # with 'maxg', det_thr before the NMS = filtering the default result afterwards
    dets, got = run(det_thr=float(t))
    after = dflt[:, 4].astype(np.float32) >= np.float32(t)
    assert 0 < after.sum() < len(dflt)
    assert same_bits(dets, dflt[after]) and np.array_equal(got, dflt_ids[after])
    # both at once: the stricter one decides; thr = +inf drops every row, thr below every probability none
    dets, got = run(thr=float(t), det_thr=float(rows[K + 30, 4]))
    assert same_bits(dets, rows[:K][wit.nms_max(rows[:K], 0.5)])
    assert len(run(thr=INF)[0]) == 0
    dets, got = run(thr=-1.0)
    assert same_bits(dets, dflt) and np.array_equal(got, dflt_ids)


# ---- the Net -------------------------------------------------------------------------------------------------------------------------
def small_net():
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_ped_cyc/mscnn-7s-576-2x", height=192, width=448, max_nms_num=200))
    synth.load_into(n, "mid")
    _, _, H, W = n.blob_shape("data")
    n.set_blob("data", synth.frame(H, W, seed=99))
    n.forward()
    return n, dict(ratios=(H / 375.0, W / 1242.0), org_hw=(375, 1242))


def _pack_to_host(ptr, nbytes):
    import ctypes as C
    torch.cuda.synchronize()
    hiprt = C.CDLL("libamdhip64.so")
    host = np.zeros(nbytes, np.uint8)
    assert hiprt.hipDeviceSynchronize() == 0
    assert hiprt.hipMemcpy(host.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(nbytes), 2) == 0      # hipMemcpyDeviceToHost
    return host


def net_calls(n, kw, cls_id):
    """The blocking, streamed and device-pack calls of a batch-1 net -> [(dets, ids)]."""
    out = [n.detect(cls_id, **kw)[:2], n.detect_image(0, cls_id, **kw)[:2]]
    segs, _ = n.detect_multi([kw], [cls_id])
    out.append(segs[0][0])
    n.detect_begin(4096, cls_id, **kw)
    out.append(n.detect_end(4096)[:2])
    ptr = n.detect_device(4096, cls_id, **kw)
    out.append(mnet.unpack_detections(_pack_to_host(ptr, mnet.detect_pack_bytes(4096)), 4096)[:2])
    R = n.blob_shape("proposals_score")[0]
    ptr = n.detect_multi_device([kw], [cls_id], R)
    segs, _ = mnet.unpack_detections_multi(_pack_to_host(ptr, mnet.detect_multi_pack_bytes(1, 1, R)), 1, 1, R)
    out.append(segs[0][0])
    return out


def test_net_setting_changes_every_detect_call_alike_and_none_restores_the_default():
    n, kw = small_net()
    fresh, _ = small_net()                                # a net on which set_nms is never called
    cls_id = 2
    rows, ids, _ = n.detect(cls_id, **dict(kw, nms_overlap=INF))
    base = net_calls(fresh, kw, cls_id)
    before = net_calls(n, kw, cls_id)
    for (d0, i0), (d1, i1) in zip(base, before):
        assert same_bits(d0, d1) and np.array_equal(i0, i1)
    keep_dflt = wit.nms_max(rows, 0.5)
    assert same_bits(base[0][0], rows[keep_dflt]) and np.array_equal(base[0][1], ids[keep_dflt])
    n.set_nms(type="max", ovr_dnm="min")
    assert n.get_nms() == dict(type="max", ovr_dnm="min", thr=None, det_thr=0.0)
    keep = wit.nms_max(rows, 0.5, greedy=False, ovr_dnm="min")
    assert keep.tobytes() != keep_dflt.tobytes() and keep.sum() > 0      # the setting matters on this frame
    for k, (dets, got) in enumerate(net_calls(n, kw, cls_id)):
        assert np.array_equal(got, ids[keep]) and same_bits(dets, rows[keep]), k
    n.set_nms(det_thr=float(rows[len(rows) // 2, 4]))     # replaces the whole setting: greedy / union again, with the plain det_thr
    want = base[0][0][:, 4].astype(np.float32) >= np.float32(rows[len(rows) // 2, 4])
    for k, (dets, got) in enumerate(net_calls(n, kw, cls_id)):
        assert same_bits(dets, base[0][0][want]) and np.array_equal(got, base[0][1][want]), k
    n.set_nms(None)
    for (d0, i0), (d1, i1) in zip(base, net_calls(n, kw, cls_id)):
        assert same_bits(d0, d1) and np.array_equal(i0, i1)


def test_net_setting_reaches_the_cascade_calls_and_the_plain_det_thr_is_refused_there_by_name():
    """detect_cascade, detect_cascade_multi and its device form under type 'max' / ovr_dnm 'min': equal to each other and to the
    witness on the rows the default call returns with nms_overlap = inf; a setting with the plain stage's det_thr makes every
    cascade call fail, naming the value, instead of ignoring it."""
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/cascade-mscnn-7s-576-2x", height=192, width=448, max_nms_num=150))
    synth.load_into(n, "mid")
    _, _, H, W = n.blob_shape("data")
    n.set_blob("data", synth.frame(H, W, seed=43))
    n.forward()
    kw = dict(ratios=(H / 375.0, W / 1242.0), org_hw=(375, 1242))
    out = ("output_bbox_1st", "cls_prob_1st", "proposals")
    rows, ids, R = n.detect_cascade(*out, cls_id=2, nms_overlap=INF, **kw)
    dflt, dflt_ids, _ = n.detect_cascade(*out, cls_id=2, **kw)
    keep_dflt = wit.nms_max(rows, 0.5)
    assert same_bits(dflt, rows[keep_dflt]) and np.array_equal(dflt_ids, ids[keep_dflt])
    n.set_nms(type="max", ovr_dnm="min")
    keep = wit.nms_max(rows, 0.5, greedy=False, ovr_dnm="min")
    assert keep.tobytes() != keep_dflt.tobytes() and keep.sum() > 0
    dets, got, _ = n.detect_cascade(*out, cls_id=2, **kw)
    assert same_bits(dets, rows[keep]) and np.array_equal(got, ids[keep])
    per_image, rois = n.detect_cascade_multi([kw], [out], [2])
    assert rois == [R] and same_bits(per_image[0][0][0][0], rows[keep]) and np.array_equal(per_image[0][0][0][1], ids[keep])
    ptr = n.detect_cascade_multi_device([kw], [out], [2], R)
    segs, _ = mnet.unpack_detections_cascade_multi(_pack_to_host(ptr, mnet.detect_cascade_multi_pack_bytes(1, 1, 1, R)), 1, 1, 1, R)
    flat = segs[0][0][0] if isinstance(segs[0][0], list) else segs[0][0]
    assert same_bits(flat[0], rows[keep]) and np.array_equal(flat[1], ids[keep])
    n.set_nms(type="max", det_thr=0.25)
    for call in (lambda: n.detect_cascade(*out, cls_id=2, **kw), lambda: n.detect_cascade_multi([kw], [out], [2]),
                 lambda: n.detect_cascade_multi_device([kw], [out], [2], R)):
        with pytest.raises(mnet.NetError, match="det_thr 0.25, which is the plain stage's"):
            call()
    n.set_nms(None)
    again, again_ids, _ = n.detect_cascade(*out, cls_id=2, **kw)
    assert same_bits(again, dflt) and np.array_equal(again_ids, dflt_ids)
