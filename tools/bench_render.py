#!/usr/bin/env python3
"""The render stage (det_render.hip) per frame of 375 x 1242, with the detections and track ids of one synthetic kitti_car forward
(seeded weights, the seeded synthetic frame, the tracker on), against the route there was before it:
  (a) the op alone: mscnn_render_detections_u8 on a device-resident frame, pack and id buffer -- device ms from hip events around
      --iters back-to-back launches after a warm-up;
  (b) the op plus the annotated frame's copy to pinned host memory -- host wall ms from an idle device to the frame on the host;
  (c) the host route: the frame, the pack and the ids copied to the host, a vectorised numpy draw (outlines and score labels by
      slicing, box after box in paint order), the annotated frame uploaded again -- host wall ms from an idle device to an idle
      device; (c') is the numpy draw alone.
(a) is also timed with --pixelate N.  The forms alternate over --rounds rounds; the median round is reported with the spread (max -
min).  Before anything is timed the numpy draw and the op are held to each other byte for byte.  --example-out FILE writes one
rendered frame (the 16 best boxes with ids, scores and track colours; their lower-scored half pixelated by a second call) for a
person to look at.
Usage: python tools/bench_render.py [--iters 200] [--warmup 20] [--rounds 5] [--quantile 0.5] [--pixelate 16] [--example-out FILE]"""
import argparse
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


def merge_pack(rows, ids):
    """A multi pack of one segment in the merge ops' form (mscnn_multi_pack_layout_of(1, cap)) and its id buffer, as uint8 / int32."""
    cap = max(len(rows), 1)
    d_at = 4 * 4 * 2
    i_at = d_at + cap * 40
    buf = np.zeros((i_at + cap * 4 + 15) // 16 * 16, np.uint8)
    buf[:d_at].view(np.int32)[:] = [1, cap, cap, 0, len(rows), len(rows), 0, 0]
    buf[d_at:i_at].view(np.float64).reshape(cap, 5)[:len(rows)] = rows
    idb = np.zeros(cap, np.int32)
    idb[:len(rows)] = ids
    return buf, idb, cap


def glyph_bitmaps():
    return {ch: np.array([[(r >> (4 - x)) & 1 for x in range(5)] for r in hipapi.render_glyph_rows(ch)], bool) for ch in "0123456789. "}


def numpy_draw(frame, rows, thr, thickness, colors, glyphs):
    """The host route's draw: the op's default setting (opaque outlines, the score at the top edge, slot colours) with numpy slices."""
    out = frame.copy()
    H, W = out.shape[:2]
    col = np.array(colors[0], np.uint8)
    ink = np.uint8(0 if 299 * int(col[0]) + 587 * int(col[1]) + 114 * int(col[2]) >= 128000 else 255)
    for x, y, w, h, s in rows[::-1]:
        if not (s >= thr and np.isfinite([x, y, w, h, s]).all()):
            continue
        L, T, R, B = int(np.floor(x + .5)), int(np.floor(y + .5)), int(np.floor(x + w + .5)) - 1, int(np.floor(y + h + .5)) - 1
        if R < L or B < T or L > W - 1 or R < 0 or T > H - 1 or B < 0:
            continue
        x0, x1, y0, y1 = max(L, 0), min(R, W - 1) + 1, max(T, 0), min(B, H - 1) + 1
        t = thickness
        out[max(T, 0):max(min(T + t, B + 1, H), 0), x0:x1] = col
        out[max(B + 1 - t, T, 0):y1, x0:x1] = col
        out[y0:y1, max(L, 0):max(min(L + t, R + 1, W), 0)] = col
        out[y0:y1, max(R + 1 - t, L, 0):x1] = col
        c = int(min(max(np.floor(s * 100 + .5), 0), 100))
        text = "1.00" if c == 100 else "0.%02d" % c
        lab = np.zeros((8, 6 * len(text)), bool)
        for i, ch in enumerate(text):
            lab[1:8, 6 * i + 1:6 * i + 6] = glyphs[ch]
        top = T - 8 if T - 8 >= 0 else T
        left = L if L + lab.shape[1] <= W else max(W - lab.shape[1], 0)
        ya, yb, xa, xb = max(top, 0), min(top + 8, H), max(left, 0), min(left + lab.shape[1], W)
        if ya < yb and xa < xb:
            m = lab[ya - top:yb - top, xa - left:xb - left]
            out[ya:yb, xa:xb] = np.where(m[:, :, None], ink, col)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quantile", type=float, default=0.5, help="show_thr = this quantile of the forward's scores (seeded weights score low)")
    ap.add_argument("--pixelate", type=int, default=16)
    ap.add_argument("--example-out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_render needs a GPU: nothing here is a time without one")

    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576"))
    synth.load_into(n, "mid")
    img = frame_u8(47)
    params = n.set_images("data", [img])
    n.forward()
    plain = n.detect_multi(params, [2])
    scores = np.sort(plain[0][0][0][0][:, 4])
    thr = float(scores[int(a.quantile * (len(scores) - 1))])
    n.set_tracker(high_thr=thr, low_thr=float(scores[0]), match_thr=0.3, max_tracks=1024)
    res = n.detect_multi(params, [2])
    rows, ids = res[0][0][0][0], n.detect_tracks()[0][0]
    drawn = int((rows[:, 4] >= thr).sum())
    colors = list(mnet.RENDER_PALETTE)

    buf, idb, cap = merge_pack(rows, ids)
    pack, idt = torch.from_numpy(buf).cuda(), torch.from_numpy(idb).cuda()
    src = torch.from_numpy(img).cuda()
    dst = torch.empty_like(src)
    host = torch.empty(img.shape, dtype=torch.uint8).pin_memory()
    host_pack, host_ids = torch.empty(buf.shape, dtype=torch.uint8).pin_memory(), torch.empty(idb.shape, dtype=torch.int32).pin_memory()
    p_def = hipapi.render_params(colors, show_thr=thr)
    p_pix = hipapi.render_params(colors, show_thr=thr, pixelate=a.pixelate)
    p_ids = hipapi.render_params(colors, show_thr=thr, label="both", color_by="id")
    glyphs = glyph_bitmaps()

    import ctypes as C
    L, st = hipapi.lib(), hipapi._stream()
    c_src, c_dst = (C.c_void_p * 1)(src.data_ptr()), (C.c_void_p * 1)(dst.data_ptr())
    c_h, c_w = (C.c_int * 1)(ORG[0]), (C.c_int * 1)(ORG[1])

    def op(p):      # (the arguments made once: the timed loop is the library call alone)
        hipapi._check(L.mscnn_render_detections_u8(C.byref(p), c_src, c_dst, c_h, c_w, 1, 1, hipapi._dev(pack), cap, hipapi._dev(idt), st))

    def op_and_copy():
        op(p_def)
        host.copy_(dst, non_blocking=True)
        torch.cuda.synchronize()

    def host_route():
        host.copy_(src, non_blocking=True)
        host_pack.copy_(pack, non_blocking=True)
        host_ids.copy_(idt, non_blocking=True)
        torch.cuda.synchronize()
        d_at = 32
        r = host_pack.numpy()[d_at:d_at + cap * 40].view(np.float64).reshape(cap, 5)[:len(rows)]
        out = numpy_draw(host.numpy(), r, thr, 2, colors, glyphs)
        dst.copy_(torch.from_numpy(out), non_blocking=True)
        torch.cuda.synchronize()
        return out

    # the two routes draw the same bytes, and the Net call the same as the op
    op(p_def)
    torch.cuda.synchronize()
    by_op = dst.cpu().numpy()
    assert np.array_equal(host_route(), by_op), "the numpy draw and the op differ"
    assert np.array_equal(n.render([img], thr=thr)[0], by_op), "Net.render and the op differ"
    assert (by_op != img).any()

    def device_ms(fn):
        for _ in range(a.warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters

    def wall_ms(fn, iters):
        for _ in range(max(a.warmup // 4, 2)):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / iters

    def draw_alone():
        numpy_draw(img, rows, thr, 2, colors, glyphs)

    forms = [("(a) op alone, device ms", lambda: device_ms(lambda: op(p_def))),
             ("(a) op alone, ids + track colours, device ms", lambda: device_ms(lambda: op(p_ids))),
             (f"(a) op alone, --pixelate {a.pixelate}, device ms", lambda: device_ms(lambda: op(p_pix))),
             ("(b) op + frame to pinned host, wall ms", lambda: wall_ms(op_and_copy, a.iters)),
             ("(c) frame, pack, ids to host + numpy draw + upload, wall ms", lambda: wall_ms(host_route, max(a.iters // 10, 5))),
             ("(c') the numpy draw alone, wall ms", lambda: wall_ms(draw_alone, max(a.iters // 10, 5)))]
    times = [[] for _ in forms]
    for r in range(a.rounds):
        for k in range(len(forms)):
            f = (k + r) % len(forms)
            times[f].append(forms[f][1]())
    print(f"# det_render.hip on one {ORG[0]} x {ORG[1]} frame ({torch.cuda.get_device_name()}): kitti_car/mscnn-7s-576, seeded weights, the seeded synthetic "
          f"frame; {len(rows)} detections in the pack, {drawn} with a score >= show_thr {thr:.4g} (quantile {a.quantile:g}) are drawn, "
          f"{int((ids > 0).sum())} carry a track id")
    print(f"# median of {a.rounds} rounds with the forms alternating, spread = max - min; {a.iters} repetitions after {a.warmup} warm-up "
          f"(a, b), {max(a.iters // 10, 5)} (c, c')")
    for (name, _), ts in zip(forms, times):
        print(f"  {name:<62s} {statistics.median(ts):9.4f}  spread {max(ts) - min(ts):.4f}")
    frame_bytes = img.size
    t_a = statistics.median(times[0])
    print(f"# (a) moves {2 * frame_bytes} frame bytes (read + write): {2 * frame_bytes / t_a / 1e6:.1f} GB/s of the device's memory bandwidth; "
          f"(c) / (b) = {statistics.median(times[4]) / statistics.median(times[3]):.1f}")

    if a.example_out:
        from PIL import Image
        thr = float(np.sort(rows[:, 4])[::-1][min(15, len(rows) - 1)])      # the 16 best boxes: a picture a person can read
        low = rows[:, 4] < np.median(rows[rows[:, 4] >= thr, 4])
        out = n.render([img], thr=thr, label="both", color_by="id", thickness=2)[0]
        # the lower-scored half of the drawn boxes pixelated: a second pack holding only those rows, drawn over the first result
        b2, i2, c2 = merge_pack(rows[low], ids[low])
        first = torch.from_numpy(out).cuda()
        second = torch.empty_like(first)
        hipapi.render_detections(hipapi.render_params(colors, show_thr=thr, label="both", color_by="id", pixelate=12), [first], 1,
                                 torch.from_numpy(b2).cuda(), c2, torch.from_numpy(i2).cuda(), out=[second])
        torch.cuda.synchronize()
        Image.fromarray(second.cpu().numpy(), "RGB").save(a.example_out, optimize=True)
        size = os.path.getsize(a.example_out)
        assert size < (1 << 20), f"{a.example_out} is {size} bytes"
        print(f"# {a.example_out}: {size} bytes")


if __name__ == "__main__":
    main()
