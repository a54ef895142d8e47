#!/usr/bin/env python3
"""Net.crops on one 375 x 1242 frame, with the detections of one synthetic kitti_car forward (seeded weights, the seeded synthetic
frame), against the route there was before it -- both of this build; the parent commit cuts no patches at all:
  (a) Net.crops: the frame on the device, the patches into a device buffer (mscnn_net_crops: the windows on the host, one views call)
      -- host wall ms from an idle device to an idle device;
  (b) the host route: the frame copied to pinned host memory (the detections are on the host already: detect_multi returned them),
      then per box the window by mnet.crop_window, a contiguous numpy copy of it, its upload and one mscnn_preprocess_u8_f32 into its
      slice of the same device buffer -- host wall ms from an idle device to an idle device;
  (b') the per-box part of (b) alone, the frame already on the host.
The forms alternate over --rounds rounds; the median round is reported with the spread (max - min).  Before anything is timed the two
routes are held to each other bit for bit.
Usage: python tools/bench_crops.py [--iters 100] [--warmup 10] [--rounds 5] [--quantile 0.5] [--size 128x64] [--context 1.0]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mscnn_amd import hipapi, net as mnet, synth, zoo  # noqa: E402

ORG = (375, 1242)


def frame_u8(seed):
    x = synth.frame(ORG[0], ORG[1], seed=seed)[0].transpose(1, 2, 0)[:, :, ::-1] + np.array([123.0, 117.0, 104.0])
    return np.ascontiguousarray(np.clip(np.round(x), 0, 255).astype(np.uint8))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quantile", type=float, default=0.5, help="thr = this quantile of the forward's scores (seeded weights score low)")
    ap.add_argument("--size", default="128x64")
    ap.add_argument("--context", type=float, default=1.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_crops needs a GPU: nothing here is a time without one")
    oh, ow = (int(v) for v in a.size.split("x"))

    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576"))
    synth.load_into(n, "mid")
    img = frame_u8(47)
    src = torch.from_numpy(img).cuda()
    params = n.set_images("data", [src])
    n.forward()
    res = n.detect_multi(params, [2])
    rows = res[0][0][0][0]
    scores = np.sort(rows[:, 4])
    thr = float(scores[int(a.quantile * (len(scores) - 1))])
    kw = dict(size=(oh, ow), thr=thr, context=a.context)
    cap = len(rows)
    out_a = torch.zeros((cap, 3, oh, ow), dtype=torch.float32, device="cuda")
    out_b = torch.zeros((cap, 3, oh, ow), dtype=torch.float32, device="cuda")
    host = torch.empty(img.shape, dtype=torch.uint8).pin_memory()
    p = mnet.crops_params(max_crops=cap, **kw)
    L, st = hipapi.lib(), hipapi._stream()
    L.mscnn_preprocess_workspace_bytes.restype = C.c_size_t
    ws = torch.empty(max(ORG[0] * ow, oh * ORG[1]) * 3 + 256, dtype=torch.uint8, device="cuda")      # (any window's intermediate fits)
    mean = (C.c_float * 3)(0.0, 0.0, 0.0)

    def crops():
        return n.crops([src], out=out_a, **kw)

    def per_box(frame):
        k = 0
        for row in rows:
            win = mnet.crop_window(p, row, ORG)
            if win is None:
                continue
            x0, y0, w, h = win
            patch = torch.from_numpy(np.ascontiguousarray(frame[y0:y0 + h, x0:x0 + w])).cuda()
            hipapi._check(L.mscnn_preprocess_u8_f32(hipapi._dev(patch), h, w, C.c_void_p(out_b[k].data_ptr()), oh, ow, mean, hipapi._dev(ws),
                                                    C.c_size_t(ws.numel()), st))
            k += 1
        torch.cuda.synchronize()
        return k

    def host_route():
        host.copy_(src, non_blocking=True)
        torch.cuda.synchronize()
        return per_box(host.numpy())

    # the two routes cut the same bits
    patches, info = crops()
    torch.cuda.synchronize()
    k = host_route()
    assert k == len(info) >= 1 and info.dropped == 0, (k, len(info), info.dropped)
    assert torch.equal(out_a[:k].view(torch.int32), out_b[:k].view(torch.int32)), "Net.crops and the host route differ"

    def wall_ms(fn, iters):
        for _ in range(max(a.warmup, 2)):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / iters

    forms = [("(a) Net.crops, device frame -> device patches, wall ms", lambda: wall_ms(crops, a.iters)),
             ("(b) frame to host + per box: slice, upload, preprocess, wall ms", lambda: wall_ms(host_route, max(a.iters // 5, 5))),
             ("(b') the per-box part alone, wall ms", lambda: wall_ms(lambda: per_box(img), max(a.iters // 5, 5)))]
    times = [[] for _ in forms]
    for r in range(a.rounds):
        for j in range(len(forms)):
            f = (j + r) % len(forms)
            times[f].append(forms[f][1]())
    w, h = np.sort(info["w"]), np.sort(info["h"])
    print(f"# Net.crops on one {ORG[0]} x {ORG[1]} frame ({torch.cuda.get_device_name()}): kitti_car/mscnn-7s-576, seeded weights, the seeded synthetic "
          f"frame; {len(rows)} detections in the pack, {k} with a score >= thr {thr:.4g} (quantile {a.quantile:g}) become patches of "
          f"{oh} x {ow}, context {a.context:g}")
    print(f"# windows (min / median / max): width {int(w[0])} / {int(w[len(w) // 2])} / {int(w[-1])}, height {int(h[0])} / {int(h[len(h) // 2])} / "
          f"{int(h[-1])} pixels")
    print(f"# median of {a.rounds} rounds with the forms alternating, spread = max - min; every repetition starts from an idle device and ends "
          f"with one; {a.iters} repetitions after {max(a.warmup, 2)} warm-up (a), {max(a.iters // 5, 5)} (b, b')")
    for (name, _), ts in zip(forms, times):
        print(f"  {name:<66s} {statistics.median(ts):9.4f}  spread {max(ts) - min(ts):.4f}")
    print(f"# (b) / (a) = {statistics.median(times[1]) / statistics.median(times[0]):.1f}")
    print("# not measured: the views kernels under a profiler, other patch sizes, host frames, the drivers end to end")


if __name__ == "__main__":
    main()
