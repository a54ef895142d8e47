#!/usr/bin/env python3
"""The views of one frame two ways: as N single forwards, and as ONE batched forward.

  singles   per view: a host crop of the frame (mirrored with [:, ::-1] when the view is), Net.set_image of it, Net.forward,
            Net.detect_merge_add -- the only way there was before Net.set_image_views; a batch-1 net
  batched   one Net.set_image_views (the frame is uploaded once, the windows are cut on the device), one Net.forward over the N
            views, one Net.detect_merge_add(..., list_of=) -- a net whose input holds N images
both between one Net.detect_merge_begin and one Net.detect_merge_end, which is part of what is timed: a window is everything a frame
costs from the decoded uint8 frame in host memory to its merged detections on the host.

Cases: caltech/mscnn-7s-480 (480 x 640 frames) and kitti_car/mscnn-7s-576 (375 x 1242), each with the frame and its mirror (N = 2)
and with 2 x 2 tiles (N = 4, --overlap pixels of overlap).  Seeded weights, a seeded frame.  Wall clock between two stream
synchronisations over --iters back-to-back frames; the forms alternate over --rounds rounds, each round starting with another form;
the median round is reported with the spread (max - min over the rounds of the same form).  The two forms see different batch sizes,
so their detections are not compared bit for bit (the project does not promise that); their counts are printed.  Nothing is asserted
on time.

Usage: python tools/bench_views.py [--iters 20] [--rounds 5] [--warmup 2] [--models ...] [--precision f32|f16x3|f16] [--overlap 32]
Whoever runs it on an MI355X keeps the output in profiles/views_batch.txt."""
import argparse
import os
import re
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mscnn_amd import net as mnet, synth, zoo  # noqa: E402

ORG_HW = {"kitti_car/mscnn-7s-576": (375, 1242), "caltech/mscnn-7s-480": (480, 640)}


def crop(img, v):
    win = img[v["y0"]:v["y0"] + v["h"], v["x0"]:v["x0"] + v["w"]]
    return np.ascontiguousarray(win[:, ::-1] if v["flip_x"] else win)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=20, help="frames per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--models", default="caltech/mscnn-7s-480,kitti_car/mscnn-7s-576")
    ap.add_argument("--precision", default="f32", choices=["f32", "f16x3", "f16"])
    ap.add_argument("--overlap", type=int, default=32, help="pixels of overlap between the 2 x 2 tiles")
    ap.add_argument("--cls-id", type=int, default=2)
    a = ap.parse_args()
    print(f"# the views of one frame as N single forwards against one batched forward ({torch.cuda.get_device_name()}, {a.precision}, \"mid\" "
          f"weights): wall ms per FRAME (begin, N views in, forward(s), add(s), end) over {a.iters} back-to-back frames between two stream "
          f"synchronisations after {a.warmup} warm-up windows, median of {a.rounds} rounds with the forms alternating, +- = max - min over the "
          "rounds of that form; ratio = singles / batched (> 1: the batch is faster)")
    print(f"# {'model':>24s} {'views':>12s} {'N':>2s} {'input':>9s} | {'singles ms':>11s} {'+-':>7s} | {'batched ms':>11s} {'+-':>7s} | ratio | "
          "dets singles / batched")
    for model in a.models.split(","):
        text = zoo.prototxt(model)
        org_hw = ORG_HW.get(model, (375, 1242))
        img = np.ascontiguousarray(np.random.default_rng(1701).integers(0, 256, org_hw + (3,), dtype=np.uint8))
        bounds = [int(v) for v in re.findall(r"max_nms_num:\s*(\d+)", text)]
        per_view = max(bounds) if bounds and max(bounds) > 0 else 2000
        one = mnet.Net(prototxt_text=text)
        synth.load_into(one, "mid")
        if a.precision != "f32":
            one.set_precision(a.precision)
        _, _, H, W = one.blob_shape("data")
        for label, (rows, cols, overlap, flip) in (("frame+mirror", (1, 1, 0, True)), ("2x2 tiles", (2, 2, a.overlap, False))):
            views, params, mviews = mnet.tile_views(org_hw, rows, cols, overlap=overlap, flip=flip, input_hw=(H, W))
            N = len(views)
            many = mnet.Net(prototxt_text=text)
            synth.load_into(many, "mid")
            if a.precision != "f32":
                many.set_precision(a.precision)
            many.reshape_input("data", (N, 3, H, W))
            cap = N * per_view
            last = {}

            def singles():
                one.detect_merge_begin(1, 1, cap)
                for v in range(N):
                    one.set_image("data", crop(img, views[v]))
                    one.forward()
                    one.detect_merge_add([params[v]], [a.cls_id], views=[mviews[v]])
                last["singles"] = len(one.detect_merge_end()[0][0][0][0])

            def batched():
                many.detect_merge_begin(1, 1, cap)
                p = many.set_image_views("data", [img], views)
                many.forward()
                many.detect_merge_add(p, [a.cls_id], views=mviews, list_of=[0] * N)
                last["batched"] = len(many.detect_merge_end()[0][0][0][0])

            def timed(call):
                def run():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.iters):
                        call()
                    torch.cuda.synchronize()
                    return (time.perf_counter() - t0) * 1e3 / a.iters
                return run

            singles(); batched()          # (the first forward runs the convolutions' own numerical checks)
            runs = {"singles": timed(singles), "batched": timed(batched)}
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
            print(f"  {model:>24s} {label:>12s} {N:>2d} {f'{H}x{W}':>9s} | {med['singles']:11.4f} {max(times['singles']) - min(times['singles']):7.4f} | "
                  f"{med['batched']:11.4f} {max(times['batched']) - min(times['batched']):7.4f} | {med['singles'] / med['batched']:5.3f} | "
                  f"{last['singles']} / {last['batched']}", flush=True)
            del many
            torch.cuda.empty_cache()
        del one
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
