#!/usr/bin/env python3
"""Net.forward() against Net.forward_rois(run_trunk=True) on the same net, the same frame and the same ROIs.

forward() runs the whole net: trunk, conv5_x / conv6_1, the proposal heads, BoxOutput with its host round trip for the row count, the
detection sub-net.  forward_rois is handed the very rows that forward's BoxOutput selected (its proposals_score blob, kept in device
memory) and runs the trunk up to conv4_3 and the sub-net around them: the layers in between never run, and R is known before anything
is enqueued.  The sub-net's outputs of the two forms are compared bit for bit first.

Cases: kitti_car/mscnn-7s-576 at the deploy's own size with the "mid" regime's own ROIs, and caltech/mscnn-7s-480.  Seeded weights, a
seeded frame.  Wall clock between two stream synchronisations over --iters back-to-back calls (forward's host round trip is part of
what is compared); the forms alternate over --rounds rounds, each round starting with another form; the median round is reported with
the spread (max - min over the rounds of the same form).  Nothing is asserted on time.

Usage: python tools/bench_forward_rois.py [--iters 30] [--rounds 5] [--warmup 3] [--models kitti_car/mscnn-7s-576,caltech/mscnn-7s-480]
Whoever runs it on an MI355X keeps the output as profiles/forward_rois.txt."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mscnn_amd import net as mnet, synth, zoo  # noqa: E402

ORG_HW = {"kitti_car/mscnn-7s-576": (375, 1242), "caltech/mscnn-7s-480": (480, 640)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=30, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--models", default="kitti_car/mscnn-7s-576,caltech/mscnn-7s-480")
    a = ap.parse_args()
    dev = torch.cuda.get_device_name()
    print(f"# forward() against forward_rois(run_trunk=True) ({dev}): the same net, frame and ROIs (\"mid\" weights, forward's own "
          f"proposals_score handed back from device memory); wall ms per call over {a.iters} back-to-back calls between two stream "
          f"synchronisations after {a.warmup} warm-up windows, median of {a.rounds} rounds with the forms alternating, +- = max - min over "
          "the rounds of that form; ratio = forward / forward_rois")
    print(f"# {'model':>26s} {'input':>10s} {'R':>5s} | {'forward ms':>12s} {'+-':>7s} | {'forward_rois ms':>15s} {'+-':>7s} | ratio")
    for model in a.models.split(","):
        n = mnet.Net(prototxt_text=zoo.prototxt(model))
        synth.load_into(n, "mid")
        _, _, H, W = n.blob_shape("data")
        n.set_blob("data", synth.frame(H, W, org_hw=ORG_HW.get(model, (375, 1242))))
        n.forward(); n.forward()          # (the first forward runs the convolutions' own numerical checks)
        ps = n.get_blob("proposals_score").reshape(-1, 6)
        want = {b: n.get_blob(b) for b in ("bbox_pred", "cls_pred")}
        rows = torch.from_numpy(ps.copy()).cuda()
        n.forward_rois(rows, "net")
        for b, ref in want.items():
            assert np.array_equal(n.get_blob(b).view(np.uint32), ref.view(np.uint32)), f"{model}: {b} differs between the two forms"

        def timed(call):
            def run():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.iters):
                    call()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3 / a.iters
            return run

        runs = {"forward": timed(n.forward), "forward_rois": timed(lambda: n.forward_rois(rows, "net"))}
        names = list(runs)
        for _ in range(a.warmup):
            for k in names:
                runs[k]()
        times = {k: [] for k in names}
        for r in range(a.rounds):
            for k in range(len(names)):
                nm = names[(k + r) % len(names)]
                times[nm].append(runs[nm]())
        med = {k: statistics.median(v) for k, v in times.items()}
        print(f"  {model:>26s} {f'{H}x{W}':>10s} {len(ps):>5d} | {med['forward']:12.4f} {max(times['forward']) - min(times['forward']):7.4f} | "
              f"{med['forward_rois']:15.4f} {max(times['forward_rois']) - min(times['forward_rois']):7.4f} | "
              f"{med['forward'] / med['forward_rois']:5.3f}", flush=True)
        del n, rows
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
