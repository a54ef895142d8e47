#!/usr/bin/env python3
"""The final detection stage alone, per step, in both forms on the same forward: B x C per-call stages (mscnn_net_detect_image, or
mscnn_net_detect for a batch-1 net) against one mscnn_net_detect_multi.  Host wall time of each form (both end with the detections
on the host), median over the steps; the two forms alternate which runs first.  Every step also checks that the two forms agree bit
for bit.  Usage: python tools/bench_final_stage.py [--steps 30] [--warmup 5] [--case caltech-f32 ...]

--cascade [--case kitti_car-cascade-b1 ...] is the same measurement for the cascade deploys: one call per (cascade output, class)
against one mscnn_net_detect_cascade_multi.  At B = 1 the per-call form is mscnn_net_detect_cascade (like for like).  At B > 1
mscnn_net_detect_cascade has no per-image form (it treats the blob as one list), so the per-call form there is a loop of per-range
op calls (hipapi.detections_cascade on each image's rows of the device blobs, row ranges read from the one-pass result outside the
timed region, each call ending with its detections on the host).

--nms-type max / --ovr-dnm min set bbNms's knobs on the net first (Net.set_nms; both forms honour the setting, so the bit-for-bit check
between them stays) and name the setting in the table's header; without them no set_nms call is made at all.

--proposals is the proposal half of the scripts' result (run_mscnn_detection.m:75-91) on the same forwards: the copy of the blob to the
host (get_blob("proposals_score")) + the numpy restatement of those lines, image after image, against one mscnn_net_proposals_multi --
both end with every image's proposals on the host, are checked bit for bit every step, and alternate which runs first.  Cases:
caltech B = 8 and kitti_car 7s-576 B = 2.  Then the step time of the RPN-only run (mscnn_net_forward_proposals) against the whole
forward on kitti_car 7s-576, B = 1, device idle before and synchronised after each, the two alternating.

--merge is the merged final stage (several forwards of a frame, one NMS: Net.detect_merge_*) against the host path it replaces, on the
same forwards: per forward get_blob of the three blobs + the numpy row transform of tests/merge_witness.py (with numpy's own exp: the
fast form a caller would write), then its sort and NMS -- against one detect_merge_add per forward and one detect_merge_end.  Only the
final-stage work is timed (host wall time, the device idle before either form starts; the forwards themselves are not), the two forms
alternate which runs first, and the whole measurement is repeated --rounds times: median of the rounds' medians and their spread.
Cases: kitti_car 7s-576 at two input sizes plus a mirrored forward, caltech 7s-480 with B = 8 likewise.

--merge --vote [THR] is box voting behind that merge (mscnn_detections_merge_vote_fwd), on the candidate lists of the same forwards:
the merge alone, the merge + the vote op, and the merge + a copy of every candidate list to the host + voting in numpy there -- what a
caller has without the op.  Each form runs from an idle device to the detections on the host; the three rotate which runs first.

--merge --soft is Soft-NMS over those candidate lists (mscnn_detections_merge_soft_fwd): the hard merge, the soft op with both methods,
unbounded and with --max-dets 300, and a copy of every candidate list to the host + a vectorised numpy Soft-NMS there -- what a caller
has without the op.  Each form runs from an idle device to the detections on the host, the forms rotate which runs first; the table
gives us per pick, and two synthetic one-list cases (4096 and 8000 candidates) price the kernel's register and streaming paths.

--merge --matrix is Matrix NMS over those candidate lists (mscnn_detections_merge_matrix_fwd): the hard merge, Soft-NMS linear, the
matrix op linear, gaussian and linear with --max-dets 300, on the two --merge --soft cases and two synthetic one-list cases (4096 and
8000 candidates); the forms rotate which runs first, and every case says whether matrix linear is below Soft-NMS linear by more than
the two spreads added, and its ratio to the hard merge.

--merge --wbf is weighted boxes fusion over those candidate lists (mscnn_detections_merge_wbf_fwd), on the cases of --merge --matrix:
the hard merge, Soft-NMS linear, Matrix NMS linear, WBF (conf avg, thr 0.55) at skip_thr 0.001, at skip_thr 0.05 and with --max-dets
300, and a copy of every candidate list to the host + a numpy WBF there (the witness's walk, the overlap vectorised over the
clusters) -- the only route there was.  The table gives the walked candidates and us per walked candidate, and every case says whether
the op is below the host route by more than the two spreads; the rows are also written to --out (profiles/detect_merge_wbf.txt).

--merge --seq is Seq-NMS over the candidate lists of a clip's frames (mscnn_detections_merge_seq_fwd): a clip is ONE forward of 8
images (kitti_car 7s-576, caltech 7s-480), frame t the seeded frame shifted 4 t pixels; the hard merge of every frame, Seq-NMS avg at
top_k 300 and 1024, and a copy of every candidate list to the host + the vectorised numpy Seq-NMS of tests/seq_witness.py there -- the
only route there was.  The table gives the boxes that entered, the iterations (sequences) and us per iteration, and every case says
whether the op is below the host route by more than the two spreads; the rows are also written to --out
(profiles/detect_merge_seq.txt).

--track is the tracker behind the final stage (mscnn_tracks_update_fwd), on the clips of --merge --seq: the final stage alone (the hard
merge of every frame of the clip, its pack read on the host), the final stage + the tracker over the clip's 8 frames in one launch
behind it (the ids read on the host too), and the final stage + the numpy tracker of tests/track_witness.py on the host's copy of the
pack -- the only route there was.  The table gives the detections, the tracks and the tracked detections, and every case says whether
the op is below the host route by more than the two spreads; the rows are also written to --out (profiles/detect_track.txt).
--track --kalman, on the same clips: the final stage alone, + the tracker with motion linear, + the tracker with a Kalman filter per
track (mscnn_tracks_update_kalman_fwd), and the pack on the host + the numpy witness of tests/track_kalman_witness.py; the filter op
is reported against the linear op of the same run, spreads included; the rows go to --out (profiles/detect_track_kalman.txt).
--track --assign, on the same clips: the final stage alone, + the tracker with the greedy walk, + the tracker with the optimal
assignment (mscnn_tracks_update_assign_fwd), each with motion linear and with the Kalman filter, the optimal form's search steps per
frame (header word 5), and one synthetic dense row, a 64 x 64 cluster; the optimal op is reported against the greedy op of the same
run; the rows go to --out (profiles/detect_track_assign.txt).
--track --streams N takes the images of ONE forward as one frame from each of N cameras (N = 0: as many as the forward has images):
(a) the final stage alone, (b) + the one-launch stream tracker (mscnn_tracks_update_streams_fwd), (c) + N single-stream
mscnn_tracks_update_fwd calls on N state buffers and N packs -- the only device route there was --, (d) the pack on the host + the
numpy witness per stream; the rows go to --out (profiles/detect_track_streams.txt).

--lib path/to/libmscnn_hip.so runs whatever leg is selected with THAT build's kernels under the Net (it is loaded first, so the Net's
calls bind to it; the per-range op calls of the batched cascade case's per-call form go through hipapi's own handle and stay this
build's).  --parent-lib path/to/libmscnn_hip.so repeats the selected leg --rounds times in child processes, this build and
that one alternating, and prints for every timed column both medians, both spreads (max - min over the rounds) and whether this
build is at or below the parent's median plus the parent's own spread."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from mscnn_amd import net as mnet, synth, zoo

CASES = {   # name: model, batch, precision, classes, original image size
    "caltech-f32-b8": ("caltech/mscnn-7s-480", 8, "f32", [2], (480, 640)),
    "caltech-f16-b8": ("caltech/mscnn-7s-480", 8, "f16", [2], (480, 640)),
    "kitti_car-7s576-b2": ("kitti_car/mscnn-7s-576", 2, "f32", [2], (375, 1242)),
    "ped_cyc-b1-cls23": ("kitti_ped_cyc/mscnn-7s-576-2x", 1, "f32", [2, 3], (375, 1242)),
}

CASCADE_CASES = {   # name: model, batch, classes, original image size
    "kitti_car-cascade-b1": ("kitti_car/cascade-mscnn-7s-576-2x", 1, [2], (375, 1242)),
    "kitti_car-cascade-b2": ("kitti_car/cascade-mscnn-7s-576-2x", 2, [2], (375, 1242)),
    "widerface-cascade-b1": ("widerface/cascade-mscnn-12s-align", 1, [2], (600, 720)),
}


def nms_set(a):
    return (a.nms_type, a.ovr_dnm) != ("maxg", "union")


def nms_label(a):
    return f", nms type {a.nms_type} / ovr_dnm {a.ovr_dnm}" if nms_set(a) else ""


def cascade_leg(a):
    import torch
    from mscnn_amd import hipapi
    print(f"# cascade final stage per step, host wall ms (median over {a.steps} steps after {a.warmup} warm-up), regime {a.regime}, "
          f"outputs 1st,2nd,3rd{nms_label(a)}")
    print(f"# {'case':22s} {'B':>2s} {'O':>2s} {'C':>2s} {'ROIs':>6s} {'dets':>5s} {'per-call ms':>12s} {'calls':>5s} {'one-pass ms':>12s} {'calls':>5s} {'saved ms':>9s}")
    for name in a.case or list(CASCADE_CASES):
        model, B, classes, org = CASCADE_CASES[name]
        n = mnet.Net(prototxt_text=zoo.prototxt(model, batch=B))
        synth.load_into(n, a.regime)
        if nms_set(a):
            if B > 1:
                sys.exit("--nms-type / --ovr-dnm with a batched cascade case: the per-call form there is the op without the net's setting")
            n.set_nms(type=a.nms_type, ovr_dnm=a.ovr_dnm)
        _, _, H, W = n.blob_shape("data")
        frames = [np.concatenate([synth.frame(H, W, seed=1701 + 13 * i + b, org_hw=org) for b in range(B)], 0) for i in range(2)]
        kw = dict(ratios=(H / float(org[0]), W / float(org[1])), org_hw=org)
        outputs = [("output_bbox_1st", "cls_prob_1st", "proposals"), ("output_bbox_2nd", "cls_prob_2nd", "proposals_2nd"),
                   ("output_bbox_3rd", "cls_prob_3rd_avg" if "cls_prob_3rd_avg" in n.blob_names else "cls_prob_3rd", "proposals_3rd")]

        def per_call(rois):
            if B == 1:
                return [[[n.detect_cascade(bb, pb, qb, cls_id=c, **kw)[:2] for c in classes] for bb, pb, qb in outputs]]
            res, row0 = [], 0
            for i in range(B):
                sl = slice(row0, row0 + rois[i])
                res.append([[tuple(t.cpu().numpy() for t in hipapi.detections_cascade(tb[sl], tp[sl], tq[sl], cls_id=c, **kw)) for c in classes]
                            for tb, tp, tq in dev_blobs])
                row0 += rois[i]
            return res

        t_call, t_multi, Rs, Ds = [], [], [], []
        for step in range(a.warmup + a.steps):
            n.set_blob("data", frames[step % 2])
            n.forward()
            _, rois = n.detect_cascade_multi([kw] * B, outputs, classes)      # (untimed: the row ranges; the forward has finished)
            if B > 1:      # the blobs on the device for the per-range op calls (copied outside the timed region)
                dev_blobs = [tuple(torch.from_numpy(n.get_blob(b).reshape(sum(rois), -1)).cuda() for b in t) for t in outputs]
                torch.cuda.synchronize()
            order = (0, 1) if step % 2 == 0 else (1, 0)
            res = [None, None]
            dt = [0.0, 0.0]
            for f in order:
                t0 = time.perf_counter()
                res[f] = per_call(rois) if f == 0 else n.detect_cascade_multi([kw] * B, outputs, classes)[0]
                dt[f] = time.perf_counter() - t0
            row0 = 0
            for i in range(B):
                for o in range(len(outputs)):
                    for c in range(len(classes)):
                        (d0, i0), (d1, i1) = res[0][i][o][c], res[1][i][o][c]
                        assert np.array_equal(d0.view(np.uint64), d1.view(np.uint64)) and np.array_equal(i0 + (row0 if B > 1 else 0), i1), (name, step, i, o, c)
                row0 += rois[i]
            if step >= a.warmup:
                t_call.append(dt[0]); t_multi.append(dt[1])
                Rs.append(sum(rois))
                Ds.append(sum(len(d) for row in res[1] for q in row for d, _ in q))
        mc, mm = 1e3 * float(np.median(t_call)), 1e3 * float(np.median(t_multi))
        print(f"  {name:22s} {B:2d} {len(outputs):2d} {len(classes):2d} {np.mean(Rs):6.0f} {np.mean(Ds):5.0f} {mc:12.3f} {B * len(outputs) * len(classes):5d} "
              f"{mm:12.3f} {1:5d} {mc - mm:9.3f}", flush=True)
        del n


def proposals_numpy(ps, params):
    """run_mscnn_detection.m:75-91 in numpy on the host copy of proposals_score [R, 6], image after image -> [(props, rows)]."""
    ps = ps.reshape(-1, 6)
    img = ps[:, 0]
    out = []
    for i, kw in enumerate(params):
        row0, row1 = np.searchsorted(img, np.float32(i), "left"), np.searchsorted(img, np.float32(i + 1), "left")
        tmp = ps[row0:row1, 1:].copy()
        tmp[:, 2] -= tmp[:, 0]; tmp[:, 3] -= tmp[:, 1]                                     # :78, single
        keep = np.flatnonzero((tmp[:, 4] >= np.float32(kw.get("proposal_thr", -10.0))) & (tmp[:, 2] != 0) & (tmp[:, 3] != 0))   # :82
        pr = tmp[keep].astype(np.float64)                                                  # :86
        pr[:, 0] /= kw["ratios"][1]; pr[:, 2] /= kw["ratios"][1]                          # :87-90
        pr[:, 1] /= kw["ratios"][0]; pr[:, 3] /= kw["ratios"][0]
        out.append((pr, (keep + row0).astype(np.int32)))
    return out


def proposals_leg(a):
    import torch
    print(f"# proposal result per step, host wall ms (median over {a.steps} steps after {a.warmup} warm-up), regime {a.regime}")
    print(f"# {'case':20s} {'B':>2s} {'ROIs':>6s} {'props':>6s} {'get_blob + numpy ms':>20s} {'one-pass ms':>12s} {'saved ms':>9s}")
    for name in a.case or ["caltech-f32-b8", "kitti_car-7s576-b2"]:
        model, B, dtype, _, org = CASES[name]
        n = mnet.Net(prototxt_text=zoo.prototxt(model, batch=B))
        synth.load_into(n, a.regime)
        if dtype != "f32":
            n.set_precision(dtype)
        _, _, H, W = n.blob_shape("data")
        frames = [np.concatenate([synth.frame(H, W, seed=1701 + 13 * i + b, org_hw=org) for b in range(B)], 0) for i in range(2)]
        params = [dict(ratios=(H / float(org[0]), W / float(org[1])))] * B
        t_np, t_one, Rs, Ps = [], [], [], []
        for step in range(a.warmup + a.steps):
            n.set_blob("data", frames[step % 2])
            n.forward()
            n.get_blob("proposals")        # (the forward has finished before either form starts)
            res = [None, None]
            dt = [0.0, 0.0]
            for f in (0, 1) if step % 2 == 0 else (1, 0):
                t0 = time.perf_counter()
                res[f] = proposals_numpy(n.get_blob("proposals_score"), params) if f == 0 else n.proposals_multi(params)[0]
                dt[f] = time.perf_counter() - t0
            for (p0, r0), (p1, r1) in zip(*res):
                assert np.array_equal(p0.view(np.uint64), p1.view(np.uint64)) and np.array_equal(r0, r1), (name, step)
            if step >= a.warmup:
                t_np.append(dt[0]); t_one.append(dt[1])
                Rs.append(n.blob_shape("proposals_score")[0]); Ps.append(sum(len(p) for p, _ in res[1]))
        m0, m1 = 1e3 * float(np.median(t_np)), 1e3 * float(np.median(t_one))
        print(f"  {name:20s} {B:2d} {np.mean(Rs):6.0f} {np.mean(Ps):6.0f} {m0:20.3f} {m1:12.3f} {m0 - m1:9.3f}", flush=True)
        del n
    model, org = "kitti_car/mscnn-7s-576", (375, 1242)
    n = mnet.Net(prototxt_text=zoo.prototxt(model))
    synth.load_into(n, a.regime)
    _, _, H, W = n.blob_shape("data")
    frames = [synth.frame(H, W, seed=1701 + 13 * i, org_hw=org) for i in range(2)]
    t = [[], []]
    for step in range(a.warmup + a.steps):
        for f in (0, 1) if step % 2 == 0 else (1, 0):
            n.set_blob("data", frames[step % 2])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n.forward() if f == 0 else n.forward_proposals()
            torch.cuda.synchronize()
            if step >= a.warmup:
                t[f].append(time.perf_counter() - t0)
    m0, m1 = 1e3 * float(np.median(t[0])), 1e3 * float(np.median(t[1]))
    print(f"# step time, host wall ms from an idle device to a synchronised one (median over {a.steps} steps after {a.warmup} warm-up), "
          f"{model} B = 1, regime {a.regime}, {n.blob_shape('proposals_score')[0]} ROIs")
    print(f"# {'whole forward ms':>18s} {'forward_proposals ms':>22s} {'saved ms':>9s}")
    print(f"  {m0:18.3f} {m1:22.3f} {m0 - m1:9.3f}", flush=True)


MERGE_CASES = {   # name: model, batch, classes, original image size, the forwards of a frame (H, W, mirrored)
    "kitti_car-7s576-2scales-flip": ("kitti_car/mscnn-7s-576", 1, [2], (375, 1242), [(576, 1920, False), (576, 1920, True), (384, 1280, False)]),
    "caltech-7s480-b8-2scales-flip": ("caltech/mscnn-7s-480", 8, [2], (480, 640), [(480, 640, False), (480, 640, True), (384, 512, False)]),
}


def merge_leg(a):
    import torch
    sys.path.insert(1, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import merge_witness as mw
    print(f"# merged final stage per frame group, host wall ms (median over {a.steps} steps after {a.warmup} warm-up; {a.rounds} rounds: median of "
          f"the medians, spread = max - min), regime {a.regime}{nms_label(a)}")
    print(f"# {'case':30s} {'B':>2s} {'fwd':>3s} {'cands':>6s} {'dets':>5s} {'get_blob + numpy ms':>20s} {'spread':>7s} {'add x fwd + merge ms':>21s} {'spread':>7s}")
    for name in a.case or list(MERGE_CASES):
        model, B, classes, org, forwards = MERGE_CASES[name]
        n = mnet.Net(prototxt_text=zoo.prototxt(model, batch=B))
        synth.load_into(n, a.regime)
        if nms_set(a):
            n.set_nms(type=a.nms_type, ovr_dnm=a.ovr_dnm)
        bound = 2000 * B * len(forwards)
        frames = {}
        for H, W, flipped in forwards:
            f = np.concatenate([synth.frame(H, W, seed=1701 + b, org_hw=org) for b in range(B)], 0)
            frames[(H, W, flipped)] = np.ascontiguousarray(f[..., ::-1]) if flipped else f
        med = [[], []]
        cands = dets = 0
        for rnd in range(a.rounds):
            t = [[], []]
            for step in range(a.warmup + a.steps):
                order = (0, 1) if step % 2 == 0 else (1, 0)
                dt = [0.0, 0.0]
                lists = [[[] for _ in classes] for _ in range(B)]
                n.detect_merge_begin(B, len(classes), bound)
                for H, W, flipped in forwards:
                    n.reshape_input("data", (B, 3, H, W))
                    n.set_blob("data", frames[(H, W, flipped)])
                    n.forward()
                    kw = dict(ratios=(H / float(org[0]), W / float(org[1])), org_hw=org)
                    view = (0.0, 0.0, 1) if flipped else None
                    for f in order:
                        torch.cuda.synchronize()      # (untimed: either form starts on an idle device)
                        t0 = time.perf_counter()
                        if f == 1:
                            n.detect_merge_add([kw] * B, classes, views=[dict(flip_x=1)] * B if flipped else None)
                        else:
                            R = n.blob_shape("proposals_score")[0]
                            bp, cp, ps = (n.get_blob(b).reshape(R, -1) for b in ("bbox_pred", "cls_pred", "proposals_score"))
                            for i in range(B):
                                r0, r1 = np.searchsorted(ps[:, 0], np.float32(i), "left"), np.searchsorted(ps[:, 0], np.float32(i + 1), "left")
                                for ci, c in enumerate(classes):
                                    rows, ids = mw.plain_rows(bp[r0:r1], cp[r0:r1], ps[r0:r1], c, exp=np.exp, **kw)
                                    lists[i][ci].append((mw.apply_view(rows, org[1], view), ids + r0))
                        dt[f] += time.perf_counter() - t0
                res = [None, None]
                for f in order:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if f == 1:
                        res[1] = n.detect_merge_end()
                    else:
                        res[0] = [[mw.merge(lists[i][ci], 0.5, a.nms_type, a.ovr_dnm) for ci in range(len(classes))] for i in range(B)]
                    dt[f] += time.perf_counter() - t0
                if step >= a.warmup:
                    t[0].append(dt[0]); t[1].append(dt[1])
                    cands = sum(c for row in res[1][1] for c in row)
                    dets = sum(len(d) for row in res[1][0] for d, _, _ in row)
                    assert cands == sum(w[3] for row in res[0] for w in row), (name, step)      # (the same rows reach both NMS)
            for f in (0, 1):
                med[f].append(1e3 * float(np.median(t[f])))
        m = [float(np.median(v)) for v in med]
        sp = [max(v) - min(v) for v in med]
        print(f"  {name:30s} {B:2d} {len(forwards):3d} {cands:6d} {dets:5d} {m[0]:20.3f} {sp[0]:7.3f} {m[1]:21.3f} {sp[1]:7.3f}", flush=True)
        del n


def host_vote(dets, cand, thr):
    """Box voting as a caller writes it in numpy today: per kept row the union overlap with every candidate of the list, then the
    prob-weighted mean of those at or over thr (at least two).  Vectorised per row; not the summation order of the device op."""
    out = dets.copy()
    xe, ye, area = cand[:, 0] + cand[:, 2], cand[:, 1] + cand[:, 3], cand[:, 2] * cand[:, 3]
    for k, A in enumerate(dets):
        iw = np.minimum(A[0] + A[2], xe) - np.maximum(A[0], cand[:, 0])
        ih = np.minimum(A[1] + A[3], ye) - np.maximum(A[1], cand[:, 1])
        o = iw * ih
        with np.errstate(divide="ignore", invalid="ignore"):
            v = (iw > 0) & (ih > 0) & (o / (A[2] * A[3] + area - o) >= thr)
        if np.count_nonzero(v) >= 2 and cand[v, 4].sum() > 0:
            out[k, :4] = (cand[v, 4:5] * cand[v, :4]).sum(0) / cand[v, 4].sum()
    return out


def merge_vote_leg(a):
    """--merge --vote: behind the same adds, (the merge alone) against (the merge + the vote op) against (the merge + a copy of every
    candidate list to the host + numpy voting there: what a caller has without the op).  All three end with the detections on the
    host; the candidate lists are those of the net's own forwards, held by hipapi.Candidates so that the host form can reach them."""
    import torch
    from mscnn_amd import hipapi
    thr = a.vote
    print(f"# box voting behind the merge (thr {thr:g}) per frame group, host wall ms from an idle device to the detections on the host (median "
          f"over {a.steps} steps after {a.warmup} warm-up; {a.rounds} rounds: median of the medians, spread = max - min), regime {a.regime}")
    print(f"# {'case':30s} {'B':>2s} {'fwd':>3s} {'cands':>6s} {'dets':>5s} {'moved':>5s} {'merge ms':>9s} {'spread':>7s} {'merge + vote ms':>16s} {'spread':>7s} "
          f"{'merge + lists to host + numpy vote ms':>38s} {'spread':>7s}")
    for name in a.case or list(MERGE_CASES):
        model, B, classes, org, forwards = MERGE_CASES[name]
        n = mnet.Net(prototxt_text=zoo.prototxt(model, batch=B))
        synth.load_into(n, a.regime)
        S, cap = B * len(classes), 2000 * B * len(forwards)
        cand = hipapi.Candidates(S, cap)
        for H, W, flipped in forwards:
            f = np.concatenate([synth.frame(H, W, seed=1701 + b, org_hw=org) for b in range(B)], 0)
            n.reshape_input("data", (B, 3, H, W))
            n.set_blob("data", np.ascontiguousarray(f[..., ::-1]) if flipped else f)
            n.forward()
            R = n.blob_shape("proposals_score")[0]
            blobs = [torch.from_numpy(n.get_blob(b).reshape(R, -1)).cuda() for b in ("bbox_pred", "cls_pred", "proposals_score")]
            segs = [dict(cls_id=c, ratios=(H / float(org[0]), W / float(org[1])), org_hw=org, nms_overlap=0.5) for _ in range(B) for c in classes]
            cand.add(*blobs, B, segs, views=[(0.0, 0.0, 1)] * B if flipped else None)
        pack = torch.zeros(hipapi.lib().mscnn_detections_multi_pack_bytes(S, S * cap), dtype=torch.uint8, device="cuda")
        ws = torch.empty(max(hipapi.lib().mscnn_detections_merge_workspace_bytes(S, cap), 1), dtype=torch.uint8, device="cuda")
        al = lambda v: (v + 255) // 256 * 256      # noqa: E731  (the candidate buffer's layout: include/mscnn_hip.h)
        o0 = al(8 * S); o1 = o0 + al(32 * S * cap)

        def on_host():
            out = cand.merge(pack=pack, ws=ws)
            cnt = cand.counts()                           # (one small copy; then of every list the filled slots only: boxes, probs)
            res = []
            for s, (dets, tags, cands) in enumerate(out):
                m = min(cnt[s][0], cap)
                box = cand.buf[o0 + 32 * s * cap:o0 + 32 * (s * cap + m)].cpu().numpy().view(np.float64).reshape(m, 4)
                prob = cand.buf[o1 + 4 * s * cap:o1 + 4 * (s * cap + m)].cpu().numpy().view(np.float32)
                res.append((host_vote(dets, np.concatenate([box, prob[:, None].astype(np.float64)], 1), thr), tags, cands))
            return res

        forms = [lambda: cand.merge(pack=pack, ws=ws), lambda: cand.merge(pack=pack, ws=ws, vote_thr=thr), on_host]
        med = [[], [], []]
        for rnd in range(a.rounds):
            t = [[], [], []]
            for step in range(a.warmup + a.steps):
                res = [None] * 3
                for f in [(0, 1, 2), (1, 2, 0), (2, 0, 1)][step % 3]:
                    torch.cuda.synchronize()      # (untimed: every form starts on an idle device)
                    t0 = time.perf_counter()
                    res[f] = forms[f]()
                    dt = time.perf_counter() - t0
                    if step >= a.warmup:
                        t[f].append(dt)
                for (d0, _, _), (d1, _, c1), (d2, _, _) in zip(*res):      # the op against the host form: the same boxes up to the summation order
                    assert np.array_equal(d0[:, 4], d1[:, 4]) and np.allclose(d1, d2, rtol=1e-12, atol=0), (name, step)
            for f in range(3):
                med[f].append(1e3 * float(np.median(t[f])))
        cands = sum(c for _, _, c in res[1])
        dets = sum(len(d) for d, _, _ in res[1])
        moved = sum(int(np.count_nonzero(np.any(d0[:, :4] != d1[:, :4], 1))) for (d0, _, _), (d1, _, _) in zip(res[0], res[1]))
        m = [float(np.median(v)) for v in med]
        sp = [max(v) - min(v) for v in med]
        print(f"  {name:30s} {B:2d} {len(forwards):3d} {cands:6d} {dets:5d} {moved:5d} {m[0]:9.3f} {sp[0]:7.3f} {m[1]:16.3f} {sp[1]:7.3f} {m[2]:38.3f} {sp[2]:7.3f}",
              flush=True)
        del n


def host_soft(cand, method, overlap, sigma, thr, max_out):
    """Soft-NMS as a caller writes it in numpy today: one pick per iteration, the decay of all live candidates vectorised."""
    box, s = cand[:, :4], cand[:, 4].copy()
    xe, ye, area = box[:, 0] + box[:, 2], box[:, 1] + box[:, 3], box[:, 2] * box[:, 3]
    live = np.ones(len(cand), bool)
    picks, scores = [], []
    while live.any() and not (max_out and len(picks) == max_out):
        m = int(np.argmax(np.where(live, s, -np.inf)))
        if not s[m] >= thr:
            break
        picks.append(m); scores.append(s[m])
        live[m] = False
        iw = np.minimum(xe[m], xe) - np.maximum(box[m, 0], box[:, 0])
        ih = np.minimum(ye[m], ye) - np.maximum(box[m, 1], box[:, 1])
        o = iw * ih
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where((iw > 0) & (ih > 0), o / (area[m] + area - o), 0.0)
        if method == "linear":
            s = np.where(live & (r > overlap), s * (1.0 - r), s)
        else:
            s = np.where(live & (r > 0), s * np.exp(-(r * r) / sigma), s)
    return np.concatenate([box[picks], np.array(scores)[:, None]], 1) if picks else np.zeros((0, 5))


def synthetic_lists(hipapi, n, seed=31):
    """One list of n candidates out of two adds: clusters of about five boxes on a 16-column grid, every row a survivor."""
    import torch
    cand = hipapi.Candidates(1, n)
    kw = dict(cls_id=2, bbox_mean=(0, 0, 0, 0), bbox_std=(0.1, 0.1, 0.2, 0.2), proposal_thr=-10.0, ratios=(1.0, 1.0), org_hw=(20000, 20000),
              nms_overlap=0.5)
    for k, rows in enumerate((n - n // 2, n // 2)):
        rng = np.random.default_rng(seed + k)
        m = rng.integers(0, max(1, rows // 5), rows)
        xy = np.stack([120 * (m % 16) + 20, 120 * (m // 16) + 20], 1) + rng.integers(-6, 7, (rows, 2))
        wh = rng.choice([14, 20, 32, 48], (rows, 2))
        props = np.concatenate([np.zeros((rows, 1)), xy, xy + wh, rng.uniform(-1, 1, (rows, 1))], 1).astype(np.float32)
        blobs = ((rng.standard_normal((rows, 8)) * 0.3).astype(np.float32), (rng.standard_normal((rows, 2)) * 2).astype(np.float32), props)
        cand.add(*[torch.from_numpy(np.ascontiguousarray(b)).cuda() for b in blobs], 1, [kw])
    return cand


def case_lists(a, hipapi, name, synthetic):
    """(B, S, cap, the filled candidate lists) of a MERGE_CASES case (its forwards run once, here) or of a synthetic one-list case."""
    import torch
    if name in synthetic:
        return 1, 1, synthetic[name], synthetic_lists(hipapi, synthetic[name])
    model, B, classes, org, forwards = MERGE_CASES[name]
    n = mnet.Net(prototxt_text=zoo.prototxt(model, batch=B))
    synth.load_into(n, a.regime)
    S, cap = B * len(classes), 2000 * B * len(forwards)
    cand = hipapi.Candidates(S, cap)
    for H, W, flipped in forwards:
        f = np.concatenate([synth.frame(H, W, seed=1701 + b, org_hw=org) for b in range(B)], 0)
        n.reshape_input("data", (B, 3, H, W))
        n.set_blob("data", np.ascontiguousarray(f[..., ::-1]) if flipped else f)
        n.forward()
        R = n.blob_shape("proposals_score")[0]
        blobs = [torch.from_numpy(n.get_blob(b).reshape(R, -1)).cuda() for b in ("bbox_pred", "cls_pred", "proposals_score")]
        segs = [dict(cls_id=c, ratios=(H / float(org[0]), W / float(org[1])), org_hw=org, nms_overlap=0.5) for _ in range(B) for c in classes]
        cand.add(*blobs, B, segs, views=[(0.0, 0.0, 1)] * B if flipped else None)
    del n
    return B, S, cap, cand


SOFT_SYNTHETIC = {"synthetic-1x4096-registers": 4096, "synthetic-1x8000-streamed": 8000}      # both paths of the kernel, one list each


def merge_soft_leg(a):
    """--merge --soft: behind the same adds, the hard merge against the soft op (both methods, unbounded and with --max-dets 300)
    against the lists copied to the host + a vectorised numpy Soft-NMS there (linear, unbounded): what a caller has without the op.
    All forms end with the detections on the host.  us / pick = a form's time over the picks of its LONGEST list (the lists run side
    by side, one workgroup each); it includes the launch and the read-back.  Two synthetic one-list cases price the kernel's two
    paths: 4096 candidates (the list in registers) and 8000 (scores and live flags streamed through the workspace)."""
    import torch
    from mscnn_amd import hipapi
    thr, sigma, md = a.soft_thr, 0.5, 300
    names = ["hard merge", "soft linear", "soft gaussian", f"linear max {md}", f"gaussian max {md}", "lists to host + numpy linear"]
    print(f"# Soft-NMS over the merged candidates (score_thr {thr:g}, sigma {sigma:g}) per frame group, host wall ms from an idle device to the "
          f"detections on the host (median over {a.steps} steps after {a.warmup} warm-up; {a.rounds} rounds: median of the medians, spread = max "
          f"- min), regime {a.regime}; picks = those of the longest list; us/pick = ms * 1000 / picks")
    print(f"# {'case':30s} {'B':>2s} {'cands':>6s} {'longest':>7s} | " + " | ".join(f"{nm:>28s} {'picks':>5s} {'spread':>6s} {'us/pick':>7s}" for nm in names))
    for name in a.case or (list(MERGE_CASES) + list(SOFT_SYNTHETIC)):
        B, S, cap, cand = case_lists(a, hipapi, name, SOFT_SYNTHETIC)
        pack = torch.zeros(hipapi.lib().mscnn_detections_multi_pack_bytes(S, S * cap), dtype=torch.uint8, device="cuda")
        ws = torch.empty(max(hipapi.lib().mscnn_detections_merge_workspace_bytes(S, cap), 1), dtype=torch.uint8, device="cuda")
        wss = torch.empty(hipapi.lib().mscnn_detections_merge_soft_workspace_bytes(S, cap), dtype=torch.uint8, device="cuda")
        al = lambda v: (v + 255) // 256 * 256      # noqa: E731  (the candidate buffer's layout: include/mscnn_hip.h)
        o0 = al(8 * S); o1 = o0 + al(32 * S * cap)

        def on_host():
            cnt = cand.counts()                           # (one small copy; then of every list the filled slots only: boxes, probs)
            res = []
            for s in range(S):
                m = min(cnt[s][0], cap)
                box = cand.buf[o0 + 32 * s * cap:o0 + 32 * (s * cap + m)].cpu().numpy().view(np.float64).reshape(m, 4)
                prob = cand.buf[o1 + 4 * s * cap:o1 + 4 * (s * cap + m)].cpu().numpy().view(np.float32)
                res.append((host_soft(np.concatenate([box, prob[:, None].astype(np.float64)], 1), "linear", 0.5, sigma, thr, 0), None, m))
            return res

        soft = lambda method, mo: (lambda: cand.merge_soft(method, sigma=sigma, score_thr=thr, max_out=mo, pack=pack, ws=wss))      # noqa: E731
        forms = [lambda: cand.merge(pack=pack, ws=ws), soft("linear", 0), soft("gaussian", 0), soft("linear", md), soft("gaussian", md), on_host]
        F = len(forms)
        med = [[] for _ in range(F)]
        for rnd in range(a.rounds):
            t = [[] for _ in range(F)]
            for step in range(a.warmup + a.steps):
                res = [None] * F
                for k in range(F):
                    f = (k + step) % F
                    torch.cuda.synchronize()      # (untimed: every form starts on an idle device)
                    t0 = time.perf_counter()
                    res[f] = forms[f]()
                    dt = time.perf_counter() - t0
                    if step >= a.warmup:
                        t[f].append(dt)
                for (d1, _, _), (d3, _, _), (d5, _, _) in zip(res[1], res[3], res[5]):      # the op against the host form, and max_out a prefix
                    assert len(d1) == len(d5) and np.allclose(d1, d5, rtol=1e-12, atol=0) and np.array_equal(d3, d1[:md]), (name, step)
            for f in range(F):
                med[f].append(1e3 * float(np.median(t[f])))
        cands = sum(c for _, _, c in res[1])
        longest = max(c for _, _, c in res[1])
        picks = [max(len(d) for d, _, _ in res[f]) for f in range(F)]
        m = [float(np.median(v)) for v in med]
        sp = [max(v) - min(v) for v in med]
        print(f"  {name:30s} {B:2d} {cands:6d} {longest:7d} | " +
              " | ".join(f"{m[f]:28.3f} {picks[f]:5d} {sp[f]:6.3f} {1e3 * m[f] / max(picks[f], 1):7.2f}" for f in range(F)), flush=True)


MATRIX_SYNTHETIC = {"synthetic-1x4096": 4096, "synthetic-1x8000": 8000}      # one list each: the tiled sort's first sizes


def merge_matrix_leg(a):
    """--merge --matrix: behind the same adds, the hard merge, Soft-NMS linear and Matrix NMS (mscnn_detections_merge_matrix_fwd):
    linear, gaussian, and linear with --max-dets 300.  All forms end with the detections on the host; they rotate within a step."""
    import torch
    from mscnn_amd import hipapi
    thr, sigma, md = a.soft_thr, 0.5, 300
    names = ["hard merge", "soft linear", "matrix linear", "matrix gaussian", f"matrix linear max {md}"]
    print(f"# Matrix NMS over the merged candidates (score_thr {thr:g}, sigma {sigma:g}) per frame group, host wall ms from an idle device to "
          f"the detections on the host (median over {a.steps} steps after {a.warmup} warm-up; {a.rounds} rounds: median of the medians, spread = "
          f"max - min), regime {a.regime}; dets = those of the longest list")
    print(f"# {'case':30s} {'B':>2s} {'cands':>6s} {'longest':>7s} | " + " | ".join(f"{nm:>22s} {'dets':>5s} {'spread':>6s}" for nm in names))
    for name in a.case or (list(MERGE_CASES) + list(MATRIX_SYNTHETIC)):
        B, S, cap, cand = case_lists(a, hipapi, name, MATRIX_SYNTHETIC)
        L = hipapi.lib()
        pack = torch.zeros(L.mscnn_detections_multi_pack_bytes(S, S * cap), dtype=torch.uint8, device="cuda")
        ws = torch.empty(max(L.mscnn_detections_merge_workspace_bytes(S, cap), 1), dtype=torch.uint8, device="cuda")
        wss = torch.empty(L.mscnn_detections_merge_soft_workspace_bytes(S, cap), dtype=torch.uint8, device="cuda")
        wsm = torch.empty(L.mscnn_detections_merge_matrix_workspace_bytes(S, cap), dtype=torch.uint8, device="cuda")
        matrix = lambda method, mo: (lambda: cand.merge_matrix(method, sigma=sigma, score_thr=thr, max_out=mo, pack=pack, ws=wsm))      # noqa: E731
        forms = [lambda: cand.merge(pack=pack, ws=ws), lambda: cand.merge_soft("linear", sigma=sigma, score_thr=thr, pack=pack, ws=wss),
                 matrix("linear", 0), matrix("gaussian", 0), matrix("linear", md)]
        F = len(forms)
        med = [[] for _ in range(F)]
        for rnd in range(a.rounds):
            t = [[] for _ in range(F)]
            for step in range(a.warmup + a.steps):
                res = [None] * F
                for k in range(F):
                    f = (k + step) % F
                    torch.cuda.synchronize()      # (untimed: every form starts on an idle device)
                    t0 = time.perf_counter()
                    res[f] = forms[f]()
                    dt = time.perf_counter() - t0
                    if step >= a.warmup:
                        t[f].append(dt)
                for (d2, _, _), (d4, _, _) in zip(res[2], res[4]):      # max_out cuts the order, it does not change it
                    assert np.array_equal(d4, d2[:md]), (name, step)
            for f in range(F):
                med[f].append(1e3 * float(np.median(t[f])))
        cands = sum(c for _, _, c in res[0])
        longest = max(c for _, _, c in res[0])
        dets = [max(len(d) for d, _, _ in res[f]) for f in range(F)]
        m = [float(np.median(v)) for v in med]
        sp = [max(v) - min(v) for v in med]
        print(f"  {name:30s} {B:2d} {cands:6d} {longest:7d} | " + " | ".join(f"{m[f]:22.3f} {dets[f]:5d} {sp[f]:6.3f}" for f in range(F)), flush=True)
        gap, both = m[1] - m[2], sp[1] + sp[2]
        print(f"# {name}: matrix linear is {'below' if gap > both else 'NOT below'} soft linear by more than the two spreads added "
              f"({m[1]:.3f} - {m[2]:.3f} = {gap:.3f} ms against {both:.3f}); matrix linear / hard merge = {m[2] / m[0]:.2f}", flush=True)


def host_wbf(cand, thr, skip_thr, expected, max_out=0):
    """Weighted boxes fusion of one list [n, 5] on the host: the walk of tests/wbf_witness.py with the overlap vectorised over the
    clusters (conf avg).  Returns (dets [D, 5], members [D])."""
    n = len(cand)
    s = cand[:, 4]
    order = np.lexsort((np.arange(n), -s))
    F, sums, members = np.zeros((n, 4)), np.zeros((n, 5)), np.zeros(n, np.int64)
    C = 0
    for i in order:
        si, B = s[i], cand[i, :4]
        if not (si >= skip_thr and si > 0):
            break
        A = F[:C]
        iw = np.minimum(A[:, 0] + A[:, 2], B[0] + B[2]) - np.maximum(A[:, 0], B[0])
        ih = np.minimum(A[:, 1] + A[:, 3], B[1] + B[3]) - np.maximum(A[:, 1], B[1])
        o = iw * ih
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where((iw > 0) & (ih > 0), o / (A[:, 2] * A[:, 3] + B[2] * B[3] - o), 0.0)
        c = int(np.argmax(r)) if C else -1
        if c < 0 or not r[c] > thr:
            sums[C] = [si, si * B[0], si * B[1], si * B[2], si * B[3]]
            members[C] = 1
            F[C] = B
            C += 1
        else:
            sums[c, 0] = sums[c, 0] + si
            sums[c, 1:] = sums[c, 1:] + si * B
            members[c] += 1
            F[c] = sums[c, 1:] / sums[c, 0]
    conf = sums[:C, 0] / members[:C] * np.minimum(members[:C], expected) / expected
    out = np.lexsort((np.arange(C), -conf))
    out = out[:max_out] if max_out > 0 else out
    return np.concatenate([F[out], conf[out, None]], 1), members[out]


def merge_wbf_leg(a):
    """--merge --wbf: behind the same adds, the hard merge, Soft-NMS linear, Matrix NMS linear and weighted boxes fusion
    (mscnn_detections_merge_wbf_fwd, conf avg, thr 0.55, expected = the forwards of the case): at skip_thr 0.001, at skip_thr 0.05, with
    --max-dets 300, and the lists copied to the host + a numpy WBF there (skip_thr 0.001) -- the only route there was.  All forms end
    with the detections on the host; they rotate within a step.  walked = the candidates that entered the longest walk of a form (the
    lists run side by side, one workgroup each); us/walked = ms * 1000 / walked includes the sort, the launches and the read-back."""
    import torch
    from mscnn_amd import hipapi
    thr, sigma, md, wthr = a.soft_thr, 0.5, 300, 0.55
    names = ["hard merge", "soft linear", "matrix linear", "wbf skip 0.001", "wbf skip 0.05", f"wbf max {md}", "lists to host + numpy wbf"]
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"# Weighted boxes fusion over the merged candidates (thr {wthr:g}, conf avg; soft / matrix score_thr {thr:g}) per frame group, host wall ms "
        f"from an idle device to the detections on the host (median over {a.steps} steps after {a.warmup} warm-up; {a.rounds} rounds: median of "
        f"the medians, spread = max - min), regime {a.regime}; dets = those of the longest output; walked = the candidates that entered the "
        f"longest walk; us/walked = ms * 1000 / walked")
    say(f"# {'case':30s} {'B':>2s} {'cands':>6s} {'longest':>7s} | " + " | ".join(f"{nm:>24s} {'dets':>5s} {'spread':>6s}" for nm in names) +
        " | walked(.001) us/walked walked(.05) us/walked")
    for name in a.case or (list(MERGE_CASES) + list(MATRIX_SYNTHETIC)):
        B, S, cap, cand = case_lists(a, hipapi, name, MATRIX_SYNTHETIC)
        T = 2 if name in MATRIX_SYNTHETIC else len(MERGE_CASES[name][4])
        L = hipapi.lib()
        pack = torch.zeros(L.mscnn_detections_multi_pack_bytes(S, S * cap), dtype=torch.uint8, device="cuda")
        members = torch.zeros(S * cap, dtype=torch.int32, device="cuda")
        ws = torch.empty(max(L.mscnn_detections_merge_workspace_bytes(S, cap), 1), dtype=torch.uint8, device="cuda")
        wss = torch.empty(L.mscnn_detections_merge_soft_workspace_bytes(S, cap), dtype=torch.uint8, device="cuda")
        wsm = torch.empty(L.mscnn_detections_merge_matrix_workspace_bytes(S, cap), dtype=torch.uint8, device="cuda")
        wsw = torch.empty(L.mscnn_detections_merge_wbf_workspace_bytes(S, cap), dtype=torch.uint8, device="cuda")
        al = lambda v: (v + 255) // 256 * 256      # noqa: E731  (the candidate buffer's layout: include/mscnn_hip.h)
        o0 = al(8 * S); o1 = o0 + al(32 * S * cap)

        def on_host():
            cnt = cand.counts()                           # (one small copy; then of every list the filled slots only: boxes, probs)
            res, mem = [], []
            for s in range(S):
                m = min(cnt[s][0], cap)
                box = cand.buf[o0 + 32 * s * cap:o0 + 32 * (s * cap + m)].cpu().numpy().view(np.float64).reshape(m, 4)
                prob = cand.buf[o1 + 4 * s * cap:o1 + 4 * (s * cap + m)].cpu().numpy().view(np.float32)
                d, mm = host_wbf(np.concatenate([box, prob[:, None].astype(np.float64)], 1), wthr, 0.001, T)
                res.append((d, None, m)); mem.append(mm)
            return res, mem

        wbf = lambda skip, mo: (lambda: cand.merge_wbf(wthr, skip_thr=skip, conf="avg", expected=T, max_out=mo, pack=pack, ws=wsw, members=members))      # noqa: E731
        forms = [lambda: (cand.merge(pack=pack, ws=ws), None), lambda: (cand.merge_soft("linear", sigma=sigma, score_thr=thr, pack=pack, ws=wss), None),
                 lambda: (cand.merge_matrix("linear", sigma=sigma, score_thr=thr, pack=pack, ws=wsm), None), wbf(0.001, 0), wbf(0.05, 0), wbf(0.001, md),
                 on_host]
        F = len(forms)
        med = [[] for _ in range(F)]
        for rnd in range(a.rounds):
            t = [[] for _ in range(F)]
            for step in range(a.warmup + a.steps):
                res = [None] * F
                for k in range(F):
                    f = (k + step) % F
                    torch.cuda.synchronize()      # (untimed: every form starts on an idle device)
                    t0 = time.perf_counter()
                    res[f] = forms[f]()
                    dt = time.perf_counter() - t0
                    if step >= a.warmup:
                        t[f].append(dt)
                for (d3, _, _), (d5, _, _), (d6, _, _), m3, m6 in zip(res[3][0], res[5][0], res[6][0], res[3][1], res[6][1]):
                    # the op against the host form (bit for bit: the same statements), and max_out a prefix
                    assert np.array_equal(d3, d6) and np.array_equal(m3, m6) and np.array_equal(d5, d3[:md]), (name, step)
            for f in range(F):
                med[f].append(1e3 * float(np.median(t[f])))
        cands = sum(c for _, _, c in res[0][0])
        longest = max(c for _, _, c in res[0][0])
        dets = [max(len(d) for d, _, _ in res[f][0]) for f in range(F)]
        walked = [max(int(m.sum()) for m in res[f][1]) for f in (3, 4)]
        m = [float(np.median(v)) for v in med]
        sp = [max(v) - min(v) for v in med]
        say(f"  {name:30s} {B:2d} {cands:6d} {longest:7d} | " + " | ".join(f"{m[f]:24.3f} {dets[f]:5d} {sp[f]:6.3f}" for f in range(F)) +
            f" | {walked[0]:12d} {1e3 * m[3] / max(walked[0], 1):9.2f} {walked[1]:11d} {1e3 * m[4] / max(walked[1], 1):9.2f}")
        say(f"# {name}: wbf skip 0.001 / lists to host + numpy wbf = {m[3] / m[6]:.3f} ({'the op is below' if m[3] + sp[3] < m[6] - sp[6] else 'the op is NOT below'} "
            f"the host route by more than the two spreads); wbf skip 0.001 / hard merge = {m[3] / m[0]:.2f}; / soft linear = {m[3] / m[1]:.2f}; "
            f"/ matrix linear = {m[3] / m[2]:.2f}")
    say("# python tools/bench_final_stage.py --merge --wbf" + f" --steps {a.steps} --warmup {a.warmup} --rounds {a.rounds}: MI355X (gfx950), one GPU, seeded "
        "weights, synthetic frames; the forwards and the add calls are not timed.  cand_cap = 2000 x B x forwards (the caltech lists are past the "
        "one-pass sort's 4032 slots and run list after list); the synthetic lists are one list each, clusters of about five boxes.")
    say("# every step asserts that the op's detections and member counts equal the host form's bit for bit, and that max_out is a prefix.")
    say("# NOT measured: the kernels alone (device events or a profiler), conf max, cascade lists, the drivers end to end, accuracy (no labels).")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


SEQ_CASES = {   # name: model, frames of the clip (one forward of B = T images), classes, original image size, net input size
    "kitti_car-7s576-clip8": ("kitti_car/mscnn-7s-576", 8, [2], (375, 1242), (576, 1920)),
    "caltech-7s480-b8-clip8": ("caltech/mscnn-7s-480", 8, [2], (480, 640), (480, 640)),
}


def seq_clip_lists(a, hipapi, name):
    """(T, K, cap, the filled candidate lists) of a SEQ_CASES case: ONE forward of T images, frame t the seeded frame shifted 4 t pixels
    to the right (a camera that pans), added once; list = frame x K + class."""
    import torch
    model, T, classes, org, (H, W) = SEQ_CASES[name]
    n = mnet.Net(prototxt_text=zoo.prototxt(model, batch=T))
    synth.load_into(n, a.regime)
    f0 = synth.frame(H, W, seed=1701, org_hw=org)
    n.reshape_input("data", (T, 3, H, W))
    n.set_blob("data", np.ascontiguousarray(np.concatenate([np.roll(f0, 4 * t, axis=-1) for t in range(T)], 0)))
    n.forward()
    R = n.blob_shape("proposals_score")[0]
    cap = 2000
    cand = hipapi.Candidates(T * len(classes), cap)
    blobs = [torch.from_numpy(n.get_blob(b).reshape(R, -1)).cuda() for b in ("bbox_pred", "cls_pred", "proposals_score")]
    segs = [dict(cls_id=c, ratios=(H / float(org[0]), W / float(org[1])), org_hw=org, nms_overlap=0.5) for _ in range(T) for c in classes]
    cand.add(*blobs, T, segs)
    del n
    return T, len(classes), cap, cand


def merge_seq_leg(a):
    """--merge --seq: behind one add of a clip's T frames, the hard merge of every frame, Seq-NMS over the clip
    (mscnn_detections_merge_seq_fwd, avg, link_thr 0.5) with top_k 300 and 1024, and the lists copied to the host + the vectorised numpy
    Seq-NMS of tests/seq_witness.py there (top_k 300) -- the only route there was.  All forms end with the detections on the host; they
    rotate within a step.  iters = the sequences of the chain (one chain per class: the loop's iterations); us/iter = ms * 1000 / iters
    includes the sort, the link launch, the launches and the read-back."""
    import torch
    from mscnn_amd import hipapi
    sys.path.insert(1, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import seq_witness as sq
    thr, link = a.soft_thr, 0.5
    names = ["hard merge", "seq avg top_k 300", "seq avg top_k 1024", "lists to host + numpy seq"]
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"# Seq-NMS over a clip's candidate lists (link_thr {link:g}, score_thr {thr:g}, rescore avg, nms_overlap 0.5) per clip, host wall ms from an "
        f"idle device to the detections on the host (median over {a.steps} steps after {a.warmup} warm-up; {a.rounds} rounds: median of the medians, "
        f"spread = max - min), regime {a.regime}; dets = those of the longest output; entered = the boxes of all frames that entered (top_k 300 / "
        f"1024); iters = the chain's sequences; us/iter = ms * 1000 / iters")
    say(f"# {'case':24s} {'T':>2s} {'cands':>6s} {'longest':>7s} | " + " | ".join(f"{nm:>25s} {'dets':>5s} {'spread':>6s}" for nm in names) +
        " | entered(300) iters us/iter entered(1024) iters us/iter longest-path")
    for name in a.case or list(SEQ_CASES):
        T, K, cap, cand = seq_clip_lists(a, hipapi, name)
        S = T * K
        L = hipapi.lib()
        pack = torch.zeros(L.mscnn_detections_multi_pack_bytes(S, S * cap), dtype=torch.uint8, device="cuda")
        ids = torch.zeros(S * cap, dtype=torch.int32, device="cuda")
        ws = torch.empty(max(L.mscnn_detections_merge_workspace_bytes(S, cap), 1), dtype=torch.uint8, device="cuda")
        wsq = torch.empty(L.mscnn_detections_merge_seq_workspace_bytes(T, K, cap, 1024), dtype=torch.uint8, device="cuda")
        al = lambda v: (v + 255) // 256 * 256      # noqa: E731  (the candidate buffer's layout: include/mscnn_hip.h)
        o0 = al(8 * S); o1 = o0 + al(32 * S * cap)
        info = {}

        def on_host():
            cnt = cand.counts()                           # (one small copy; then of every list the filled slots only: boxes, probs)
            lists = []
            for s in range(S):
                m = min(cnt[s][0], cap)
                box = cand.buf[o0 + 32 * s * cap:o0 + 32 * (s * cap + m)].cpu().numpy().view(np.float64).reshape(m, 4)
                prob = cand.buf[o1 + 4 * s * cap:o1 + 4 * (s * cap + m)].cpu().numpy().view(np.float32)
                lists.append(np.concatenate([box, prob[:, None].astype(np.float64)], 1))
            res, seqs = [None] * S, [None] * S
            for k in range(K):
                rows, tr = sq.seq_nms(lists[k::K], link, [0.5] * T, thr, 300, sq.AVG, 0)
                info["longest"] = max(info.get("longest", 0), max(len(p) for p in tr["paths"]))
                for t, (d, slots, q) in enumerate(rows):
                    res[t * K + k], seqs[t * K + k] = (d, None, len(lists[t * K + k])), q.astype(np.int32)
            return res, seqs

        seq = lambda top_k: (lambda: cand.merge_seq(link, T, score_thr=thr, top_k=top_k, rescore="avg", pack=pack, ws=wsq, seq=ids))      # noqa: E731
        forms = [lambda: (cand.merge(pack=pack, ws=ws), None), seq(300), seq(1024), on_host]
        F = len(forms)
        med = [[] for _ in range(F)]
        for rnd in range(a.rounds):
            t = [[] for _ in range(F)]
            for step in range(a.warmup + a.steps):
                res = [None] * F
                for k in range(F):
                    f = (k + step) % F
                    torch.cuda.synchronize()      # (untimed: every form starts on an idle device)
                    t0 = time.perf_counter()
                    res[f] = forms[f]()
                    dt = time.perf_counter() - t0
                    if step >= a.warmup:
                        t[f].append(dt)
                for (d1, _, _), (d3, _, _), q1, q3 in zip(res[1][0], res[3][0], res[1][1], res[3][1]):
                    assert np.array_equal(d1, d3) and np.array_equal(q1, q3), (name, step)      # the op against the host form, bit for bit
            for f in range(F):
                med[f].append(1e3 * float(np.median(t[f])))
        cands = sum(c for _, _, c in res[0][0])
        longest = max(c for _, _, c in res[0][0])
        dets = [max(len(d) for d, _, _ in res[f][0]) for f in range(F)]
        iters = [max(max([int(q.max()) + 1 for q in res[f][1][k::K] if len(q)] or [0]) for k in range(K)) for f in (1, 2)]
        cnt = cand.counts()
        entered = []
        for top_k in (300, 1024):
            e = 0
            for s in range(S):
                m = min(cnt[s][0], cap)
                prob = cand.buf[o1 + 4 * s * cap:o1 + 4 * (s * cap + m)].cpu().numpy().view(np.float32)
                e += min(int(np.count_nonzero(prob.astype(np.float64) >= thr)), top_k)
            entered.append(e)
        m = [float(np.median(v)) for v in med]
        sp = [max(v) - min(v) for v in med]
        say(f"  {name:24s} {T:2d} {cands:6d} {longest:7d} | " + " | ".join(f"{m[f]:25.3f} {dets[f]:5d} {sp[f]:6.3f}" for f in range(F)) +
            f" | {entered[0]:12d} {iters[0]:5d} {1e3 * m[1] / max(iters[0], 1):7.2f} {entered[1]:13d} {iters[1]:5d} {1e3 * m[2] / max(iters[1], 1):7.2f}"
            f" {info.get('longest', 0):12d}")
        say(f"# {name}: seq top_k 300 / lists to host + numpy seq = {m[1] / m[3]:.3f} ({'the op is below' if m[1] + sp[1] < m[3] - sp[3] else 'the op is NOT below'} "
            f"the host route by more than the two spreads); seq top_k 300 / hard merge = {m[1] / m[0]:.2f}; top_k 1024 / top_k 300 = {m[2] / m[1]:.2f}")
    say("# python tools/bench_final_stage.py --merge --seq" + f" --steps {a.steps} --warmup {a.warmup} --rounds {a.rounds}: MI355X (gfx950), one GPU, seeded "
        "weights; a clip is ONE forward of T = 8 images, frame t the seeded synthetic frame shifted 4 t pixels (a panning camera); the forward and the "
        "add call are not timed.  cand_cap = 2000 per frame and class (the one-pass sort).")
    say("# every step asserts that the op's detections and sequence ids (top_k 300) equal the host form's bit for bit.")
    say("# NOT measured: the kernels alone (device events or a profiler), rescore max, clips of other lengths, more than one class (chains run side by "
        "side, one workgroup each), lists past 4032 slots (sorted list after list), the cascade lists, the drivers end to end, real video, accuracy "
        "(no labels).")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def track_leg(a):
    """--track: on the clips --merge --seq uses, behind one add of a clip's T frames: the final stage alone (the hard merge, its pack read
    on the host), the final stage + the tracker (mscnn_tracks_update_fwd over the clip's T frames in one launch behind the merge, on a
    freshly reset table; the ids read on the host too), and the final stage + the witness-grade numpy tracker of tests/track_witness.py on
    the host's copy of the pack -- the only route there was.  All forms end with the detections (and ids) on the host; they rotate within
    a step."""
    import torch
    from mscnn_amd import hipapi
    sys.path.insert(1, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import track_witness as tw
    kw = dict(high_thr=0.5, low_thr=0.1, match_thr=0.3, match_thr_low=0.5, motion="linear", vel_gain=0.5, max_age=30, min_hits=1)
    M = 256
    p, cp = tw.params(**kw), hipapi.track_params(**kw)
    names = ["final stage alone", "final stage + tracker", "pack to host + numpy tracker"]
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"# the tracker behind the final stage (high_thr {kw['high_thr']:g}, low_thr {kw['low_thr']:g}, match_thr {kw['match_thr']:g}, match_thr_low "
        f"{kw['match_thr_low']:g}, motion linear, max_tracks {M}) per clip, host wall ms from an idle device to the detections (and ids) on the host "
        f"(median over {a.steps} steps after {a.warmup} warm-up; {a.rounds} rounds: median of the medians, spread = max - min), regime {a.regime}; "
        f"dets = the detections of all frames; tracks = the table's tracks after the clip; tracked = the detections with an id > 0")
    say(f"# {'case':24s} {'T':>2s} {'dets':>5s} {'tracks':>6s} {'tracked':>7s} | " + " | ".join(f"{nm:>28s} {'spread':>6s}" for nm in names) + " | tracker ms")
    for name in a.case or list(SEQ_CASES):
        T, K, cap, cand = seq_clip_lists(a, hipapi, name)
        S = T * K
        L = hipapi.lib()
        pack = torch.zeros(L.mscnn_detections_multi_pack_bytes(S, S * cap), dtype=torch.uint8, device="cuda")
        ws = torch.empty(max(L.mscnn_detections_merge_workspace_bytes(S, cap), 1), dtype=torch.uint8, device="cuda")
        state = hipapi.tracks_state_new(K, M)
        ids = torch.zeros(S * cap, dtype=torch.int32, device="cuda")

        def alone():
            return cand.merge(pack=pack, ws=ws), None, None

        def on_device():
            out = cand.merge(pack=pack, ws=ws)
            hipapi.tracks_update(cp, T, K, pack, S * cap, state, M, None, ids)
            h = ids.cpu().numpy()      # (synchronises: the ids are on the host)
            return out, [h[s * cap:s * cap + len(d)] for s, (d, _, _) in enumerate(out)], None

        def on_host():
            out = cand.merge(pack=pack, ws=ws)
            slots = [tw.new_slot() for _ in range(K)]
            got = tw.run(slots, [[out[t * K + k][0] for k in range(K)] for t in range(T)], p, M)
            return out, [got[s // K][s % K] for s in range(S)], slots

        forms = [alone, on_device, on_host]
        F = len(forms)
        med = [[] for _ in range(F)]
        for rnd in range(a.rounds):
            t = [[] for _ in range(F)]
            for step in range(a.warmup + a.steps):
                res = [None] * F
                for k in range(F):
                    f = (k + step) % F
                    hipapi._check(L.mscnn_tracks_state_reset(hipapi._dev(state), K, M, hipapi._stream()))      # (untimed: every clip starts a stream)
                    torch.cuda.synchronize()      # (untimed: every form starts on an idle device)
                    t0 = time.perf_counter()
                    res[f] = forms[f]()
                    dt = time.perf_counter() - t0
                    if step >= a.warmup:
                        t[f].append(dt)
                assert all(np.array_equal(x, y) for x, y in zip(res[1][1], res[2][1])), (name, step)      # the op against the host form, bit for bit
            for f in range(F):
                med[f].append(1e3 * float(np.median(t[f])))
        dets = sum(len(d) for d, _, _ in res[0][0])
        tracks = sum(sl["n"] for sl in res[2][2])
        tracked = sum(int(np.count_nonzero(i)) for i in res[1][1])
        m = [float(np.median(v)) for v in med]
        sp = [max(v) - min(v) for v in med]
        say(f"  {name:24s} {T:2d} {dets:5d} {tracks:6d} {tracked:7d} | " + " | ".join(f"{m[f]:28.3f} {sp[f]:6.3f}" for f in range(F)) + f" | {m[1] - m[0]:10.3f}")
        say(f"# {name}: (final stage + tracker) - final stage alone = {m[1] - m[0]:.3f} ms per clip of {T} frames; + tracker / + numpy tracker = {m[1] / m[2]:.3f} "
            f"({'the op is below' if m[1] + sp[1] < m[2] - sp[2] else 'the op is NOT below'} the host route by more than the two spreads)")
    say("# python tools/bench_final_stage.py --track" + f" --steps {a.steps} --warmup {a.warmup} --rounds {a.rounds}: MI355X (gfx950), one GPU, seeded weights; a "
        "clip is ONE forward of T = 8 images, frame t the seeded synthetic frame shifted 4 t pixels (a panning camera); the forward and the add call are "
        "not timed, the table is reset before every timed form.  The tracker's column is a difference of two host wall times: its launch is enqueued "
        "behind the read of the pack, so it holds a second synchronisation and the copy of the id buffer (one int32 per pack row) as well.")
    say("# every step asserts that the op's ids equal the host form's bit for bit.")
    say("# NOT measured: the kernel alone (device events or a profiler), one frame per call (a stream), more than one class (slots run side by side, one "
        "workgroup each), tables near max_tracks = 1024, the Net calls and the drivers end to end, real video, accuracy (no labels).")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def track_kalman_leg(a):
    """--track --kalman: on the clips of --track, behind one add of a clip's T frames: the final stage alone, + the tracker with motion
    linear (mscnn_tracks_update_fwd), + the tracker with a Kalman filter per track (mscnn_tracks_update_kalman_fwd, motion none, the
    default stds), and the pack on the host + the numpy witness of tests/track_kalman_witness.py.  Every form starts on an idle device
    and a freshly reset table and ends with the detections (and ids) on the host; the forms rotate within a step."""
    import torch
    from mscnn_amd import hipapi
    sys.path.insert(1, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import track_kalman_witness as kw
    import track_witness as tw
    kws = dict(high_thr=0.5, low_thr=0.1, match_thr=0.3, match_thr_low=0.5, vel_gain=0.5, max_age=30, min_hits=1)
    M = 256
    p_none, cp_lin, cp_none = tw.params(motion="none", **kws), hipapi.track_params(motion="linear", **kws), hipapi.track_params(motion="none", **kws)
    kp, ckp = kw.kparams(), hipapi.track_kalman_params()
    names = ["final stage alone", "+ tracker, motion linear", "+ tracker, Kalman filter", "pack to host + numpy witness"]
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"# a Kalman filter per track behind the final stage (high_thr {kws['high_thr']:g}, low_thr {kws['low_thr']:g}, match_thr {kws['match_thr']:g}, "
        f"match_thr_low {kws['match_thr_low']:g}, max_tracks {M}; the filter's default stds) per clip, host wall ms from an idle device to the detections "
        f"(and ids) on the host (median over {a.steps} steps after {a.warmup} warm-up; {a.rounds} rounds: median of the medians, spread = max - min), "
        f"regime {a.regime}; dets = the detections of all frames; tracks = the filter's table after the clip; tracked = its detections with an id > 0")
    say(f"# {'case':24s} {'T':>2s} {'dets':>5s} {'tracks':>6s} {'tracked':>7s} | " + " | ".join(f"{nm:>28s} {'spread':>6s}" for nm in names) +
        " | linear ms | kalman ms")
    for name in a.case or list(SEQ_CASES):
        T, K, cap, cand = seq_clip_lists(a, hipapi, name)
        S = T * K
        L = hipapi.lib()
        pack = torch.zeros(L.mscnn_detections_multi_pack_bytes(S, S * cap), dtype=torch.uint8, device="cuda")
        ws = torch.empty(max(L.mscnn_detections_merge_workspace_bytes(S, cap), 1), dtype=torch.uint8, device="cuda")
        state = hipapi.tracks_state_new(K, M)
        filt = torch.zeros(hipapi.tracks_kalman_state_bytes(K, M), dtype=torch.uint8, device="cuda")
        ids = torch.zeros(S * cap, dtype=torch.int32, device="cuda")

        def ids_of(out):
            h = ids.cpu().numpy()      # (synchronises: the ids are on the host)
            return [h[s * cap:s * cap + len(d)] for s, (d, _, _) in enumerate(out)]

        def alone():
            return cand.merge(pack=pack, ws=ws), None, None

        def linear():
            out = cand.merge(pack=pack, ws=ws)
            hipapi.tracks_update(cp_lin, T, K, pack, S * cap, state, M, None, ids)
            return out, ids_of(out), None

        def kalman():
            out = cand.merge(pack=pack, ws=ws)
            hipapi.tracks_update_kalman(cp_none, ckp, T, K, 1, None, pack, S * cap, state, filt, M, None, None, ids)
            return out, ids_of(out), None

        def on_host():
            out = cand.merge(pack=pack, ws=ws)
            slots = [tw.new_slot() for _ in range(K)]
            got = kw.run(slots, [[out[t * K + k][0] for k in range(K)] for t in range(T)], p_none, kp, M)
            return out, [got[s // K][s % K] for s in range(S)], slots

        forms = [alone, linear, kalman, on_host]
        F = len(forms)
        med = [[] for _ in range(F)]
        for rnd in range(a.rounds):
            t = [[] for _ in range(F)]
            for step in range(a.warmup + a.steps):
                res = [None] * F
                for k in range(F):
                    f = (k + step) % F
                    hipapi._check(L.mscnn_tracks_state_reset(hipapi._dev(state), K, M, hipapi._stream()))      # (untimed: every clip starts a stream)
                    torch.cuda.synchronize()      # (untimed: every form starts on an idle device)
                    t0 = time.perf_counter()
                    res[f] = forms[f]()
                    dt = time.perf_counter() - t0
                    if step >= a.warmup:
                        t[f].append(dt)
                assert all(np.array_equal(x, y) for x, y in zip(res[2][1], res[3][1])), (name, step)      # the filter op against the witness, bit for bit
            for f in range(F):
                med[f].append(1e3 * float(np.median(t[f])))
        dets = sum(len(d) for d, _, _ in res[0][0])
        tracks = sum(sl["n"] for sl in res[3][2])
        tracked = sum(int(np.count_nonzero(i)) for i in res[2][1])
        m = [float(np.median(v)) for v in med]
        sp = [max(v) - min(v) for v in med]
        lin, kal = m[1] - m[0], m[2] - m[0]
        say(f"  {name:24s} {T:2d} {dets:5d} {tracks:6d} {tracked:7d} | " + " | ".join(f"{m[f]:28.3f} {sp[f]:6.3f}" for f in range(F)) +
            f" | {lin:9.3f} | {kal:9.3f}")
        say(f"# {name}: the filter op costs {kal:.3f} ms per clip of {T} frames on top of the final stage, the linear op {lin:.3f} ms: {kal / lin:.2f}x "
            f"(spreads {sp[2]:.3f} and {sp[1]:.3f} ms); + Kalman filter / + numpy witness = {m[2] / m[3]:.3f}")
    say("# python tools/bench_final_stage.py --track --kalman" + f" --steps {a.steps} --warmup {a.warmup} --rounds {a.rounds}: MI355X (gfx950), one GPU, seeded "
        "weights; the clips, the add call and the resets as in profiles/detect_track.txt.  Both tracker columns are differences of two host wall times and "
        "hold a second synchronisation and the copy of the id buffer.  Every step asserts that the filter op's ids equal the witness's bit for bit.")
    say("# NOT measured: the kernels alone (device events or a profiler), one frame per call, more than one class, several streams, tables near "
        "max_tracks = 1024 (the filter kernel's 154 KB of LDS allow one workgroup per CU), the Net calls and the drivers end to end, real video, "
        "accuracy (no labels).")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def track_assign_leg(a):
    """--track --assign: on the clips of --track, behind one add of a clip's T frames: the final stage alone, + the tracker with the
    greedy walk and + the tracker with the optimal assignment (mscnn_tracks_update_assign_fwd), each with motion linear and with a
    Kalman filter per track; the optimal form's search steps per frame from header word 5.  Then one synthetic dense row: a 64 x 64
    cluster (centres sigma 2 px, size 40 px), the two ops alone.  Every form starts on an idle device and a freshly reset table and
    ends with the ids on the host; the forms rotate within a step."""
    import torch
    from mscnn_amd import hipapi
    sys.path.insert(1, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import track_assign_witness as aw
    import track_kalman_witness as kw
    import track_witness as tw
    kws = dict(high_thr=0.5, low_thr=0.1, match_thr=0.3, match_thr_low=0.5, vel_gain=0.5, max_age=30, min_hits=1)
    M = 256
    cp_lin, cp_none, ckp = hipapi.track_params(motion="linear", **kws), hipapi.track_params(motion="none", **kws), hipapi.track_kalman_params()
    names = ["final stage alone", "+ greedy, linear", "+ optimal, linear", "+ greedy, Kalman", "+ optimal, Kalman"]
    lines = []
    L = hipapi.lib()

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def measure(forms, reset, check):
        F = len(forms)
        med = [[] for _ in range(F)]
        res = [None] * F
        for rnd in range(a.rounds):
            t = [[] for _ in range(F)]
            for step in range(a.warmup + a.steps):
                for k in range(F):
                    f = (k + step) % F
                    reset()                        # (untimed: every clip starts a stream)
                    torch.cuda.synchronize()       # (untimed: every form starts on an idle device)
                    t0 = time.perf_counter()
                    res[f] = forms[f]()
                    dt = time.perf_counter() - t0
                    if step >= a.warmup:
                        t[f].append(dt)
                check(res)
            for f in range(F):
                med[f].append(1e3 * float(np.median(t[f])))
        return [float(np.median(v)) for v in med], [max(v) - min(v) for v in med], res

    say(f"# the optimal assignment beside the greedy walk behind the final stage (high_thr {kws['high_thr']:g}, low_thr {kws['low_thr']:g}, match_thr "
        f"{kws['match_thr']:g}, match_thr_low {kws['match_thr_low']:g}, max_tracks {M}) per clip, host wall ms from an idle device to the ids on the host "
        f"(median over {a.steps} steps after {a.warmup} warm-up; {a.rounds} rounds: median of the medians, spread = max - min), regime {a.regime}; "
        "steps/frame = header word 5 after the clip over its frames, summed over the slots; differ = detections whose id differs between the two forms")
    say(f"# {'case':24s} {'T':>2s} {'dets':>5s} | " + " | ".join(f"{nm:>18s} {'spread':>6s}" for nm in names) +
        " | greedy ms | optimal ms | steps/frame | greedy K ms | optimal K ms | steps/frame K | differ")
    for name in a.case or list(SEQ_CASES):
        T, K, cap, cand = seq_clip_lists(a, hipapi, name)
        S = T * K
        pack = torch.zeros(L.mscnn_detections_multi_pack_bytes(S, S * cap), dtype=torch.uint8, device="cuda")
        ws = torch.empty(max(L.mscnn_detections_merge_workspace_bytes(S, cap), 1), dtype=torch.uint8, device="cuda")
        state = hipapi.tracks_state_new(K, M)
        filt = torch.zeros(hipapi.tracks_kalman_state_bytes(K, M), dtype=torch.uint8, device="cuda")
        ids = torch.zeros(S * cap, dtype=torch.int32, device="cuda")

        def form(cp, kp_, assign):
            def run():
                out = cand.merge(pack=pack, ws=ws)
                hipapi.tracks_update_assign(cp, kp_, assign, T, K, 1, None, pack, S * cap, state, M, filter_in=filt if kp_ is not None else None, ids=ids)
                h = ids.cpu().numpy()      # (synchronises: the ids are on the host)
                return out, [h[s * cap:s * cap + len(d)].copy() for s, (d, _, _) in enumerate(out)], sum(hipapi.tracks_state_steps(state.cpu().numpy(), K, M))
            return run

        forms = [lambda: (cand.merge(pack=pack, ws=ws), None, 0), form(cp_lin, None, "greedy"), form(cp_lin, None, "optimal"),
                 form(cp_none, ckp, "greedy"), form(cp_none, ckp, "optimal")]

        def check(res):
            assert res[1][2] == 0 and res[3][2] == 0, "the greedy form wrote header word 5"

        m, sp, res = measure(forms, lambda: hipapi._check(L.mscnn_tracks_state_reset(hipapi._dev(state), K, M, hipapi._stream())), check)
        dets = sum(len(d) for d, _, _ in res[0][0])
        differ = sum(int(np.count_nonzero(x != y)) for x, y in zip(res[1][1], res[2][1]))
        say(f"  {name:24s} {T:2d} {dets:5d} | " + " | ".join(f"{m[f]:18.3f} {sp[f]:6.3f}" for f in range(5)) +
            f" | {m[1] - m[0]:9.3f} | {m[2] - m[0]:10.3f} | {res[2][2] / T:11.1f} | {m[3] - m[0]:11.3f} | {m[4] - m[0]:12.3f} | {res[4][2] / T:13.1f} | {differ:6d}")
        say(f"# {name}: the optimal op costs {m[2] - m[0]:.3f} ms per clip of {T} frames on top of the final stage where the greedy op costs {m[1] - m[0]:.3f} ms "
            f"({(m[2] - m[0]) / (m[1] - m[0]):.2f}x); with the Kalman filter {m[4] - m[0]:.3f} against {m[3] - m[0]:.3f} ms ({(m[4] - m[0]) / (m[3] - m[0]):.2f}x)")
    # the synthetic dense row: one slot, frame 1 = 64 boxes that start 64 tracks, frame 2 = 64 boxes around the same point
    n = 64
    A, B = aw.dense(np.random.default_rng(n), n)
    rows = lambda b: np.concatenate([b, np.full((n, 1), 0.9)], axis=1)
    frames = [[rows(A)], [rows(B)]]
    buf, offs, cap = tw.pack_bytes(frames, n)
    pack = torch.from_numpy(buf).cuda()
    state = hipapi.tracks_state_new(1, M)
    ids = torch.zeros(cap, dtype=torch.int32, device="cuda")

    def dense_form(assign):
        def run():
            hipapi.tracks_update_assign(cp_none, None, assign, 2, 1, 1, None, pack, cap, state, M, ids=ids)
            return ids.cpu().numpy().copy(), hipapi.tracks_state_steps(state.cpu().numpy(), 1, M)[0]
        return run
    slots = [tw.new_slot()]
    want = aw.run(slots, frames, tw.params(motion="none", **kws), M)

    def check_dense(res):
        assert np.array_equal(res[1][0][offs[1]:offs[1] + n], want[1][0]) and res[1][1] == slots[0]["steps"], "the optimal op is not the witness"
    m, sp, res = measure([dense_form("greedy"), dense_form("optimal")], lambda: hipapi._check(L.mscnn_tracks_state_reset(hipapi._dev(state), 1, M, hipapi._stream())),
                         check_dense)
    kept = [int(np.count_nonzero((r[0][offs[1]:offs[1] + n] > 0) & (r[0][offs[1]:offs[1] + n] <= n))) for r in res]
    say(f"# synthetic dense cluster, {n} tracks x {n} detections (centres sigma 2 px around one point, size 40 px, motion none), the tracker op alone, two "
        f"frames (the first starts the tracks): greedy {m[0]:.3f} ms (spread {sp[0]:.3f}), optimal {m[1]:.3f} ms (spread {sp[1]:.3f}), {res[1][1]} steps; "
        f"detections of frame 2 that keep one of the {n} ids: greedy {kept[0]}, optimal {kept[1]}")
    say("# python tools/bench_final_stage.py --track --assign" + f" --steps {a.steps} --warmup {a.warmup} --rounds {a.rounds}: MI355X (gfx950), one GPU, seeded "
        "weights; the clips, the add call and the resets as in profiles/detect_track.txt.  The tracker columns are differences of two host wall times and "
        "hold a second synchronisation, the copy of the id buffer and (all four alike) a copy of the state for word 5.  Every step asserts that the greedy "
        "forms leave word 5 at 0 and that the dense row's optimal ids and steps equal tests/track_assign_witness.py.")
    say("# NOT measured: the kernels alone (device events or a profiler), the cost of one step, one frame per call, more than one class, several streams, "
        "tables near max_tracks = 1024, a dense table above 64 x 64 (a dense 1024 x 1024 one could take about 5e5 steps), the Net calls and the drivers end "
        "to end, real video, accuracy (no labels).")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


STREAM_CASES = {   # name: (a SEQ_CASES entry: model, images of the one forward = cameras, classes, original image size, net input size)
    "caltech-7s480-b8": ("caltech/mscnn-7s-480", 8, [2], (480, 640), (480, 640)),
    "kitti_car-7s576-b4": ("kitti_car/mscnn-7s-576", 4, [2], (375, 1242), (576, 1920)),
}


def track_streams_leg(a):
    """--track --streams N: the images of ONE forward are one frame from each of N cameras (frame b belongs to stream b % N).  Behind one
    add of the forward's images: (a) the final stage alone (the hard merge, its pack read on the host); (b) the final stage + the
    stream tracker, ONE launch (mscnn_tracks_update_streams_fwd); (c) the final stage + N single-stream mscnn_tracks_update_fwd calls,
    one per camera, each on a state buffer and a pack of its own -- the only device route the parent commit has; the N packs hold the
    same rows and are made ahead, untimed, which favours (c) --; (d) the pack on the host + the numpy witness per stream.  Every form
    starts from tables that have seen these frames once (a running system: every track finds its detection again); all forms end with
    the detections (and ids) on the host; they rotate within a step."""
    import copy
    import torch
    from mscnn_amd import hipapi
    sys.path.insert(1, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import track_streams_witness as sw
    import track_witness as tw
    kw = dict(high_thr=0.5, low_thr=0.1, match_thr=0.3, match_thr_low=0.5, motion="linear", vel_gain=0.5, max_age=30, min_hits=1)
    M = 256
    p, cp = tw.params(**kw), hipapi.track_params(**kw)
    names = ["(a) final stage alone", "(b) + stream tracker, 1 launch", "(c) + N single-stream calls", "(d) pack to host + numpy"]
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"# the tracker for a batch of cameras behind the final stage (high_thr {kw['high_thr']:g}, low_thr {kw['low_thr']:g}, match_thr {kw['match_thr']:g}, "
        f"match_thr_low {kw['match_thr_low']:g}, motion linear, max_tracks {M}) per forward, host wall ms from an idle device to the detections (and ids) "
        f"on the host (median over {a.steps} steps after {a.warmup} warm-up; {a.rounds} rounds: median of the medians, spread = max - min), regime "
        f"{a.regime}; B = the images of the forward; N = the streams; dets = the detections of all images; tracks = the tables' tracks; tracked = the "
        f"detections with an id > 0")
    say(f"# {'case':22s} {'B':>2s} {'N':>2s} {'dets':>5s} {'tracks':>6s} {'tracked':>7s} | " + " | ".join(f"{nm:>30s} {'spread':>6s}" for nm in names) +
        " | (b)-(a) ms | (c)-(a) ms")
    SEQ_CASES.update(STREAM_CASES)
    for name in a.case or list(STREAM_CASES):
        T, K, cap, cand = seq_clip_lists(a, hipapi, name)
        N = a.streams or T
        stream_of = [b % N for b in range(T)]
        S = T * K
        L = hipapi.lib()
        pack = torch.zeros(L.mscnn_detections_multi_pack_bytes(S, S * cap), dtype=torch.uint8, device="cuda")
        ws = torch.empty(max(L.mscnn_detections_merge_workspace_bytes(S, cap), 1), dtype=torch.uint8, device="cuda")
        ids = torch.zeros(S * cap, dtype=torch.int32, device="cuda")
        out0 = cand.merge(pack=pack, ws=ws)
        frames = [[out0[t * K + k][0] for k in range(K)] for t in range(T)]
        # the tables after these frames once: (b)'s state, (c)'s N states, (d)'s dicts
        base = hipapi.tracks_state_new(N * K, M)
        hipapi.tracks_update_streams(cp, T, K, N, stream_of, pack, S * cap, base, M)
        state = base.clone()
        base_tables = sw.new_tables(N, K)
        sw.run(base_tables, frames, stream_of, p, M)
        per, where = sw.split(frames, stream_of, N)
        packs, base_n, state_n, ids_n = [], [], [], []
        for s in range(N):      # stream s alone: its frames in a pack of their own (the same rows), its own state and ids
            buf, _, rows_s = tw.pack_bytes(per[s], cap, "merge", fill=0)
            packs.append((torch.from_numpy(buf).cuda(), rows_s))
            b = hipapi.tracks_state_new(K, M)
            hipapi.tracks_update(cp, len(per[s]), K, packs[s][0], rows_s, b, M)
            base_n.append(b)
            state_n.append(b.clone())
            ids_n.append(torch.zeros(rows_s, dtype=torch.int32, device="cuda"))
        tables = [None]

        def alone():
            return cand.merge(pack=pack, ws=ws), None

        def one_launch():
            out = cand.merge(pack=pack, ws=ws)
            hipapi.tracks_update_streams(cp, T, K, N, stream_of, pack, S * cap, state, M, None, ids)
            h = ids.cpu().numpy()      # (synchronises: the ids are on the host)
            return out, [h[s * cap:s * cap + len(d)] for s, (d, _, _) in enumerate(out)]

        def n_calls():
            out = cand.merge(pack=pack, ws=ws)
            for s in range(N):
                hipapi.tracks_update(cp, len(per[s]), K, packs[s][0], packs[s][1], state_n[s], M, None, ids_n[s])
            got = [None] * S
            for s in range(N):
                h = ids_n[s].cpu().numpy()
                for i, t in enumerate(where[s]):
                    for k in range(K):
                        got[t * K + k] = h[(i * K + k) * cap:(i * K + k) * cap + len(out[t * K + k][0])]
            return out, got

        def on_host():
            out = cand.merge(pack=pack, ws=ws)
            got = sw.run(tables[0], [[out[t * K + k][0] for k in range(K)] for t in range(T)], stream_of, p, M)
            return out, [got[s // K][s % K] for s in range(S)]

        forms = [alone, one_launch, n_calls, on_host]
        F = len(forms)
        med = [[] for _ in range(F)]
        for rnd in range(a.rounds):
            t = [[] for _ in range(F)]
            for step in range(a.warmup + a.steps):
                res = [None] * F
                for k in range(F):
                    f = (k + step) % F
                    state.copy_(base)      # (untimed: every form starts from the same tables)
                    for s in range(N):
                        state_n[s].copy_(base_n[s])
                    tables[0] = copy.deepcopy(base_tables)
                    torch.cuda.synchronize()      # (untimed: every form starts on an idle device)
                    t0 = time.perf_counter()
                    res[f] = forms[f]()
                    dt = time.perf_counter() - t0
                    if step >= a.warmup:
                        t[f].append(dt)
                for other in (2, 3):      # the one launch against the N calls and against the host form, bit for bit
                    assert all(np.array_equal(x, y) for x, y in zip(res[1][1], res[other][1])), (name, step, other)
            for f in range(F):
                med[f].append(1e3 * float(np.median(t[f])))
        dets = sum(len(d) for d, _, _ in res[0][0])
        tracks = sum(sl["n"] for tab in tables[0] for sl in tab)
        tracked = sum(int(np.count_nonzero(i)) for i in res[1][1])
        m = [float(np.median(v)) for v in med]
        sp = [max(v) - min(v) for v in med]
        say(f"  {name:22s} {T:2d} {N:2d} {dets:5d} {tracks:6d} {tracked:7d} | " + " | ".join(f"{m[f]:30.3f} {sp[f]:6.3f}" for f in range(F)) +
            f" | {m[1] - m[0]:10.3f} | {m[2] - m[0]:10.3f}")
        say(f"# {name}: the one launch adds {m[1] - m[0]:.3f} ms to the final stage, the {N} single-stream calls add {m[2] - m[0]:.3f} ms; (b) / (c) = {m[1] / m[2]:.3f} "
            f"({'(b) is below' if m[1] + sp[1] < m[2] - sp[2] else '(b) is NOT below'} (c) by more than the two spreads); (b) / (d) = {m[1] / m[3]:.3f}")
    say("# python tools/bench_final_stage.py --track --streams " + f"{a.streams} --steps {a.steps} --warmup {a.warmup} --rounds {a.rounds}: MI355X (gfx950), one GPU, "
        "seeded weights; ONE forward of B images, image b the seeded synthetic frame shifted 4 b pixels, stream b % N (--streams 0: N = B); the forward "
        "and the add call are not timed; every form starts from tables that have seen the same frames once.  (b)-(a) and (c)-(a) are differences of "
        "two host wall times: the launches are enqueued behind the read of the pack, so they hold a second synchronisation and the copy of the id "
        "buffer(s) as well; (c) reads N id buffers, and its N packs were made ahead (untimed).")
    say("# every step asserts that the ids of (b), (c) and (d) are equal bit for bit.")
    say("# NOT measured: the kernel alone (device events or a profiler), more than one class (K = 1: one workgroup per stream), more than one frame per "
        "stream in a call, streams without a frame, more than 8 streams, tables near max_tracks = 1024, the Net calls (set_frame_streams, detect_multi) "
        "and the drivers end to end, real video, accuracy (no labels).")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def use_lib(path):
    """The kernels of another build of libmscnn_hip.so under this build's Net: loaded first and globally, the Net library's calls bind
    to it (checked on one final-stage symbol)."""
    import ctypes as C
    path = os.path.abspath(path)
    other = C.CDLL(path, mode=C.RTLD_GLOBAL)
    mnet.lib()
    addr = lambda h: C.cast(h.mscnn_detections_multi_nms_fwd, C.c_void_p).value      # noqa: E731
    assert addr(C.CDLL(None)) == addr(other), "the process did not bind the final stage to " + path
    print(f"# kernels of {path}")


def ab_leg(a, argv):
    """--parent-lib: the selected leg in child processes, this build and the parent's alternating; every timed column of every row."""
    import subprocess
    child = [x for i, x in enumerate(argv) if x != "--parent-lib" and (i == 0 or argv[i - 1] != "--parent-lib")]
    runs = {"new": [], "parent": []}
    labels = None
    for rnd in range(a.rounds):
        for which in (("new", "parent") if rnd % 2 == 0 else ("parent", "new")):
            cmd = [sys.executable, os.path.abspath(__file__)] + child + (["--lib", a.parent_lib] if which == "parent" else [])
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(f"{' '.join(cmd)} failed with status {r.returncode}:\n{r.stderr[-2000:]}")
            out = r.stdout
            rows = {}
            for line in out.splitlines():
                tok = line.split()
                if line.startswith("  ") and tok:
                    vals = [float(v) for v in tok if "." in v]
                    rows[tok[0] if "." not in tok[0] else "step-time"] = vals[:-1]      # (the last column is the difference of the others)
            runs[which].append(rows)
            labels = labels or list(rows)
    print(f"# {' '.join(child) or '(plain leg)'}: {a.rounds} rounds per build, alternating; ms; spread = max - min over the rounds")
    print(f"# {'row':24s} {'col':>3s} {'new median':>11s} {'spread':>7s} {'parent median':>14s} {'spread':>7s}  at or below parent median + spread")
    ok = True
    for row in labels:
        for col in range(len(runs["new"][0][row])):
            v = {w: [r[row][col] for r in runs[w]] for w in runs}
            mn, mp = float(np.median(v["new"])), float(np.median(v["parent"]))
            sn, spp = max(v["new"]) - min(v["new"]), max(v["parent"]) - min(v["parent"])
            good = mn <= mp + spp
            ok &= good
            print(f"  {row:24s} {col:3d} {mn:11.3f} {sn:7.3f} {mp:14.3f} {spp:7.3f}  {'yes' if good else 'NO'}", flush=True)
    print("# every row at or below the parent's median + spread" if ok else "# NOT every row is at or below the parent's median + spread")


ap = argparse.ArgumentParser()
ap.add_argument("--merge", action="store_true", help="several forwards of a frame, one NMS: get_blob + numpy per forward against "
                "detect_merge_add per forward + detect_merge_end")
ap.add_argument("--vote", nargs="?", type=float, const=0.5, default=None, metavar="THR", help="with --merge: the merge alone, the merge "
                "+ the vote op, and the merge + every candidate list to the host + numpy voting")
ap.add_argument("--soft", action="store_true", help="with --merge: the hard merge, the Soft-NMS op (linear and gaussian, unbounded and with "
                "--max-dets 300) and every candidate list to the host + a vectorised numpy Soft-NMS; us per pick")
ap.add_argument("--matrix", action="store_true", help="with --merge: the hard merge, Soft-NMS linear and the Matrix NMS op (linear, gaussian, "
                "linear with --max-dets 300) on the --merge --soft cases and two synthetic lists")
ap.add_argument("--wbf", action="store_true", help="with --merge: the hard merge, Soft-NMS linear, Matrix NMS linear and the weighted boxes "
                "fusion op (skip_thr 0.001 and 0.05, and with --max-dets 300) against every candidate list to the host + a numpy WBF; us per "
                "walked candidate; the rows also go to --out")
ap.add_argument("--seq", action="store_true", help="with --merge: per clip of 8 frames the hard merge, the Seq-NMS op (avg, top_k 300 and 1024) "
                "and every candidate list to the host + a vectorised numpy Seq-NMS; us per iteration; the rows also go to --out")
ap.add_argument("--track", action="store_true", help="on the clips of --merge --seq: the final stage alone, the final stage + the tracker op, and "
                "the pack on the host + the numpy tracker of tests/track_witness.py; the rows also go to --out")
ap.add_argument("--kalman", action="store_true", help="with --track: the final stage alone, + the tracker with motion linear, + the tracker with a "
                "Kalman filter per track (mscnn_tracks_update_kalman_fwd), the pack on the host + tests/track_kalman_witness.py; the rows also go "
                "to --out (profiles/detect_track_kalman.txt)")
ap.add_argument("--assign", action="store_true", help="with --track: the final stage alone, + the tracker with the greedy walk and + the tracker with "
                "the optimal assignment (mscnn_tracks_update_assign_fwd), motion linear and Kalman filter, the search steps per frame, and one "
                "synthetic dense 64 x 64 cluster; the rows also go to --out (profiles/detect_track_assign.txt)")
ap.add_argument("--streams", type=int, default=None, metavar="N", help="with --track: the images of one forward as one frame from each of N "
                "cameras (0: as many as images): the final stage alone, + the one-launch stream tracker, + N single-stream calls, the pack on "
                "the host + the numpy witness per stream; the rows also go to --out")
ap.add_argument("--out", default=None, help="--merge --wbf / --merge --seq / --track: the file the rows are written to (default: "
                "profiles/detect_merge_wbf.txt / profiles/detect_merge_seq.txt / profiles/detect_track.txt, with --streams "
                "profiles/detect_track_streams.txt; '' = none)")
ap.add_argument("--soft-thr", type=float, default=0.001, help="--merge --soft / --matrix / --wbf: the score threshold of Soft-NMS and Matrix NMS")
ap.add_argument("--rounds", type=int, default=3, help="--merge / --parent-lib: repetitions of the whole measurement")
ap.add_argument("--lib", default="", help="run with the kernels of this libmscnn_hip.so under the Net")
ap.add_argument("--parent-lib", default="", help="A/B of the selected leg against this libmscnn_hip.so, alternating child processes")
ap.add_argument("--proposals", action="store_true", help="the proposal result: get_blob + numpy against one proposals_multi, and the "
                "RPN-only run against the whole forward")
ap.add_argument("--cascade", action="store_true", help="the cascade deploys: per-call detect_cascade against one detect_cascade_multi")
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--case", nargs="*", default=None)
ap.add_argument("--regime", default="mid")
ap.add_argument("--form", choices=("both", "call", "multi"), default="both",
                help="one form alone (under a tracer: the launches and synchronisations of that form per step)")
ap.add_argument("--nms-type", default="maxg", choices=("maxg", "max"), help="bbNms's type for both forms (Net.set_nms)")
ap.add_argument("--ovr-dnm", default="union", choices=("union", "min"), help="bbNms's overlap denominator for both forms")
a = ap.parse_args()
if a.out is None:
    a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                         "detect_track_streams.txt" if a.track and a.streams is not None else "detect_track_kalman.txt" if a.track and a.kalman else "detect_track_assign.txt" if a.track and a.assign else "detect_track.txt" if a.track else "detect_merge_seq.txt" if a.seq else "detect_merge_wbf.txt")
if a.parent_lib:
    ab_leg(a, sys.argv[1:])
    sys.exit(0)
if a.lib:
    use_lib(a.lib)
if a.streams is not None and not (a.track and 0 <= a.streams <= 256):
    ap.error(f"--streams {a.streams} belongs to --track and lies inside [0, 256]")
if a.kalman and not (a.track and a.streams is None):
    ap.error("--kalman belongs to --track (without --streams)")
if a.assign and not (a.track and a.streams is None and not a.kalman):
    ap.error("--assign belongs to --track (without --streams and --kalman)")
if a.track and a.assign:
    track_assign_leg(a)
    sys.exit(0)
if a.track and a.kalman:
    track_kalman_leg(a)
    sys.exit(0)
if a.track and a.streams is not None:
    track_streams_leg(a)
    sys.exit(0)
if a.track:
    track_leg(a)
    sys.exit(0)
if a.merge and a.vote is not None:
    merge_vote_leg(a)
    sys.exit(0)
if a.merge and a.soft:
    merge_soft_leg(a)
    sys.exit(0)
if a.merge and a.matrix:
    merge_matrix_leg(a)
    sys.exit(0)
if a.merge and a.wbf:
    merge_wbf_leg(a)
    sys.exit(0)
if a.merge and a.seq:
    merge_seq_leg(a)
    sys.exit(0)
if a.merge:
    merge_leg(a)
    sys.exit(0)
if a.cascade:
    cascade_leg(a)
    sys.exit(0)
if a.proposals:
    proposals_leg(a)
    sys.exit(0)
if a.case is None:
    a.case = list(CASES)

print(f"# final stage per step, host wall ms (median over {a.steps} steps after {a.warmup} warm-up), regime {a.regime}{nms_label(a)}")
print(f"# {'case':20s} {'B':>2s} {'C':>2s} {'ROIs':>6s} {'dets':>5s} {'per-call ms':>12s} {'calls':>5s} {'one-pass ms':>12s} {'calls':>5s} {'saved ms':>9s}")
for name in a.case:
    model, B, dtype, classes, org = CASES[name]
    n = mnet.Net(prototxt_text=zoo.prototxt(model, batch=B))
    synth.load_into(n, a.regime)
    if dtype != "f32":
        n.set_precision(dtype)
    if nms_set(a):
        n.set_nms(type=a.nms_type, ovr_dnm=a.ovr_dnm)
    _, _, H, W = n.blob_shape("data")
    frames = [np.concatenate([synth.frame(H, W, seed=1701 + 13 * i + b, org_hw=org) for b in range(B)], 0) for i in range(2)]
    kw = dict(ratios=(H / float(org[0]), W / float(org[1])), org_hw=org)
    params = [kw] * B

    def per_call():
        if B == 1:
            return [[n.detect(c, **kw)[:2] for c in classes]]
        return [[n.detect_image(i, c, **kw)[:2] for c in classes] for i in range(B)]

    t_call, t_multi, Rs, Ds = [], [], [], []
    for step in range(a.warmup + a.steps):
        n.set_blob("data", frames[step % 2])
        n.forward()
        n.get_blob("proposals_score")        # (the forward has finished before either form starts)
        order = (0, 1) if step % 2 == 0 else (1, 0)
        res = [None, None]
        dt = [0.0, 0.0]
        for f in [f for f in order if a.form == "both" or f == ("call", "multi").index(a.form)]:
            t0 = time.perf_counter()
            res[f] = per_call() if f == 0 else n.detect_multi(params, classes)[0]
            dt[f] = time.perf_counter() - t0
        for i in range(B if a.form == "both" else 0):
            for c in range(len(classes)):
                (d0, i0), (d1, i1) = res[0][i][c], res[1][i][c]
                assert np.array_equal(d0.view(np.uint64), d1.view(np.uint64)) and np.array_equal(i0, i1), (name, step, i, c)
        if step >= a.warmup:
            t_call.append(dt[0]); t_multi.append(dt[1])
            Rs.append(n.blob_shape("proposals_score")[0])
            Ds.append(sum(len(d) for row in res[1 if res[1] is not None else 0] for d, _ in row))
    mc, mm = 1e3 * float(np.median(t_call)), 1e3 * float(np.median(t_multi))      # (a form not run: 0)
    print(f"  {name:20s} {B:2d} {len(classes):2d} {np.mean(Rs):6.0f} {np.mean(Ds):5.0f} {mc:12.3f} {B * len(classes):5d} {mm:12.3f} {1:5d} {mc - mm:9.3f}",
          flush=True)
    del n
