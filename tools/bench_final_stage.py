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
forward on kitti_car 7s-576, B = 1, device idle before and synchronised after each, the two alternating."""
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


ap = argparse.ArgumentParser()
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
