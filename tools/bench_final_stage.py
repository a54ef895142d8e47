#!/usr/bin/env python3
"""The final detection stage alone, per step, in both forms on the same forward: B x C per-call stages (mscnn_net_detect_image, or
mscnn_net_detect for a batch-1 net) against one mscnn_net_detect_multi.  Host wall time of each form (both end with the detections
on the host), median over the steps; the two forms alternate which runs first.  Every step also checks that the two forms agree bit
for bit.  Usage: python tools/bench_final_stage.py [--steps 30] [--warmup 5] [--case caltech-f32 ...]"""
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

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--case", nargs="*", default=list(CASES))
ap.add_argument("--regime", default="mid")
ap.add_argument("--form", choices=("both", "call", "multi"), default="both",
                help="one form alone (under a tracer: the launches and synchronisations of that form per step)")
a = ap.parse_args()

print(f"# final stage per step, host wall ms (median over {a.steps} steps after {a.warmup} warm-up), regime {a.regime}")
print(f"# {'case':20s} {'B':>2s} {'C':>2s} {'ROIs':>6s} {'dets':>5s} {'per-call ms':>12s} {'calls':>5s} {'one-pass ms':>12s} {'calls':>5s} {'saved ms':>9s}")
for name in a.case:
    model, B, dtype, classes, org = CASES[name]
    n = mnet.Net(prototxt_text=zoo.prototxt(model, batch=B))
    synth.load_into(n, a.regime)
    if dtype != "f32":
        n.set_precision(dtype)
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
