#!/usr/bin/env python3
"""The ROIAlign head of the WiderFace cascade (roi_grid_org / roi_pool_org / roi_grid_ctx / roi_pool_ctx / roi_pool) in its two forms.

Op level: the layer chain -- mscnn_roialign_fwd_f32, mscnn_pool2d_fwd_f32 (AVE 2x2 / stride 1), both twice, then the Concat's two
mscnn_concat_channels_f32 copies: six launches, four intermediate blobs -- against mscnn_roialign_ave_pair_fwd_f32 (one launch, the
result alone) at the deploy's shapes: C = 512, 5 x 5 bins, scale 1/8, paddings 0 / 0.25, a 64 x 64 map (a 512 x 512 frame) with
R = 150, 700, 3000 ROIs and a 384 x 384 map (a 3072 x 3072 frame) with R = 3000.  Device time from hip events around back-to-back calls
after a warm-up, all buffers allocated once; the number of calls per window is chosen so that a window lasts >= --window seconds.  The
forms alternate over --rounds rounds (each round starts with another form); the median round is reported with the spread (max - min
over the rounds of the same form).  The two forms are compared bit for bit first.  --parent-lib times the chain of another build of
libmscnn_hip.so (e.g. the parent commit's) on the same buffers, loaded beside this one.

Net level: widerface/cascade-mscnn-12s-align at 512 x 512 with seeded weights, the whole forward (host round trips of the three
BoxOutput / DecodeBBox stages included: wall clock between two stream synchronisations) with Net.set_roialign_one_pass off and on,
two nets with the same weights on the same frame, alternating in the same way.

Usage: python tools/bench_roialign_head.py [--window 0.6] [--warmup 5] [--rounds 5] [--net-iters 30] [--parent-lib path/to/libmscnn_hip.so]
                                           [--skip-net] [--skip-ops]"""
import argparse
import ctypes as C
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mscnn_amd import hipapi, net as mnet, synth, zoo  # noqa: E402

PH = PW = 5
SCALE, PAD_A, PAD_B = 0.125, 0.0, 0.25
CH = 512
OP_CASES = [(64, 64, 150), (64, 64, 700), (64, 64, 3000), (384, 384, 3000)]      # feature map H, W and the number of ROIs


def bind(L):
    L.mscnn_last_error.restype = C.c_char_p
    L.mscnn_roialign_fwd_f32.argtypes = [C.c_void_p] * 3 + [C.c_int] * 7 + [C.c_float, C.c_float, C.c_void_p]
    L.mscnn_pool2d_fwd_f32.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 11 + [C.c_void_p]
    L.mscnn_concat_channels_f32.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]
    return L


def rois_for(gen, R, H, W):
    """Face-sized boxes (8 .. 1/3 of the frame's side), fractional, some over the border, in image coordinates."""
    ih, iw = H / SCALE, W / SCALE
    side = torch.exp(torch.empty(R).uniform_(math.log(8.0), math.log(min(ih, iw) / 3.0), generator=gen))
    aspect = torch.empty(R).uniform_(0.7, 1.4, generator=gen)
    w, h = side, side * aspect
    x1 = torch.empty(R).uniform_(-0.05, 0.95, generator=gen) * iw
    y1 = torch.empty(R).uniform_(-0.05, 0.95, generator=gen) * ih
    return torch.stack([torch.zeros(R), x1, y1, x1 + w, y1 + h], 1).float().cuda()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--window", type=float, default=0.6, help="seconds a timed window of back-to-back calls lasts at least")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--net-iters", type=int, default=30)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--skip-net", action="store_true")
    ap.add_argument("--skip-ops", action="store_true")
    a = ap.parse_args()

    L = hipapi.lib()
    P = bind(C.CDLL(os.path.abspath(a.parent_lib))) if a.parent_lib else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    gen = torch.Generator().manual_seed(1701)
    dev = torch.cuda.get_device_name()

    def window(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    def alternate(forms, iters_of):
        """forms: name -> callable.  -> name -> per-call ms of every round."""
        names = list(forms)
        for n in names:
            for _ in range(a.warmup):
                forms[n]()
        times = {n: [] for n in names}
        for r in range(a.rounds):
            for k in range(len(names)):
                n = names[(k + r) % len(names)]
                times[n].append(window(forms[n], iters_of[n]))
        return times

    if not a.skip_ops:
        print(f"# ROIAlign head, op level ({dev}): C = {CH}, {PH} x {PW} bins, scale {SCALE}, paddings {PAD_A} / {PAD_B}; device ms per call "
              f"from hip events over back-to-back calls (windows >= {a.window} s) after {a.warmup} warm-up calls, median of {a.rounds} "
              "rounds with the forms alternating, +- = max - min over the rounds of that form")
        print("# chain = roialign, pool2d AVE 2x2 / 1, roialign, pool2d, concat x 2 (6 launches, grid and pooled blobs in memory); "
              "one-pass = roialign_ave_pair (1 launch); ratio = chain / one-pass")
        names = ["chain", "one-pass"] + (["parent chain"] if P else [])
        print(f"# {'map':>9s} {'R':>5s}" + "".join(f" | {n + ' ms':>15s} {'+-':>7s} {'calls':>5s}" for n in names) + " | ratio")
        for H, W, R in OP_CASES:
            feat = torch.randn((1, CH, H, W), generator=gen, dtype=torch.float32).clamp_(min=0).cuda()
            rois = rois_for(gen, R, H, W)
            grid = [torch.empty((R, CH, PH + 1, PW + 1), dtype=torch.float32, device="cuda") for _ in range(2)]
            pooled = [torch.empty((R, CH, PH, PW), dtype=torch.float32, device="cuda") for _ in range(2)]
            out_chain = torch.empty((R, 2 * CH, PH, PW), dtype=torch.float32, device="cuda")
            out_pair = torch.empty_like(out_chain)

            def chain_of(lib):
                def run():
                    rc = 0
                    for k, pad in enumerate((PAD_A, PAD_B)):
                        rc |= lib.mscnn_roialign_fwd_f32(feat.data_ptr(), rois.data_ptr(), grid[k].data_ptr(), R, 1, CH, H, W, PH, PW, SCALE, pad, st)
                        rc |= lib.mscnn_pool2d_fwd_f32(grid[k].data_ptr(), pooled[k].data_ptr(), R, CH, PH + 1, PW + 1, 2, 2, 0, 0, 1, 1, 1, st)
                    for k in range(2):
                        rc |= lib.mscnn_concat_channels_f32(pooled[k].data_ptr(), out_chain.data_ptr(), R, CH, PH * PW, 2 * CH, k * CH, st)
                    if rc != 0:
                        raise RuntimeError(lib.mscnn_last_error().decode())
                return run

            def one_pass():
                rc = L.mscnn_roialign_ave_pair_fwd_f32(feat.data_ptr(), rois.data_ptr(), out_pair.data_ptr(), R, 1, CH, H, W, PH, PW, SCALE,
                                                       PAD_A, 0, PAD_B, CH, 2 * CH, st)
                if rc != 0:
                    raise RuntimeError(L.mscnn_last_error().decode())

            forms = {"chain": chain_of(L), "one-pass": one_pass}
            if P:
                forms["parent chain"] = chain_of(P)
            out_chain.fill_(float("nan")); out_pair.fill_(float("nan"))
            forms["chain"](); forms["one-pass"]()
            torch.cuda.synchronize()
            assert torch.equal(out_chain, out_pair), "the chain and the one-pass op differ"
            if P:
                out_chain.fill_(float("nan"))
                forms["parent chain"]()
                torch.cuda.synchronize()
                assert torch.equal(out_chain, out_pair), "the parent's chain and the one-pass op differ"
            iters_of = {}
            for n, fn in forms.items():
                per_call = window(fn, 3) / 1e3
                iters_of[n] = max(20, int(math.ceil(a.window / max(per_call, 1e-6))))
            times = alternate(forms, iters_of)
            row = f"  {f'{H}x{W}':>9s} {R:>5d}"
            for n in names:
                row += f" | {statistics.median(times[n]):15.4f} {max(times[n]) - min(times[n]):7.4f} {iters_of[n]:>5d}"
            row += f" | {statistics.median(times['chain']) / statistics.median(times['one-pass']):5.2f}"
            print(row, flush=True)
            del feat, rois, grid, pooled, out_chain, out_pair
            torch.cuda.empty_cache()

    if not a.skip_net:
        model, side = "widerface/cascade-mscnn-12s-align", 512
        x = synth.frame(side, side, org_hw=(side, side))
        nets = {}
        for name, on in (("five layers", False), ("one-pass", True)):
            n = mnet.Net(prototxt_text=zoo.prototxt(model, height=side, width=side))
            synth.load_into(n, "mid")
            n.set_roialign_one_pass(on)
            n.set_blob("data", x)
            n.forward(); n.forward()          # (the first forward runs the convolutions' own numerical checks)
            nets[name] = n
        off, on = nets["five layers"], nets["one-pass"]
        heads = on.roialign_pairs()
        assert [on.layer_kernel(i) for i in heads] == ["roialign_ave_pair"] * 3 and [off.layer_kernel(i) for i in heads] == [""] * 3
        for b in ("roi_pool", "roi_pool_2nd", "roi_pool_3rd", "output_bbox_3rd", "cls_prob_3rd_avg"):
            assert np.array_equal(on.get_blob(b), off.get_blob(b)), b
        rows = [on.blob_shape(b)[0] for b in ("proposals", "proposals_2nd", "proposals_3rd")]

        def forwards(n):
            def run():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.net_iters):
                    n.forward()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3 / a.net_iters
            return run

        runs = {k: forwards(n) for k, n in nets.items()}
        names = list(runs)
        for k in names:
            runs[k]()
        times = {k: [] for k in names}
        for r in range(a.rounds):
            for k in range(len(names)):
                nm = names[(k + r) % len(names)]
                times[nm].append(runs[nm]())
        print(f"# Net level ({dev}): {model} at {side} x {side}, seeded weights, ROIs per stage {rows}; wall ms per whole forward over "
              f"{a.net_iters} forwards between two stream synchronisations, median of {a.rounds} rounds with the forms alternating, "
              "+- = max - min over the rounds of that form; ratio = five layers / one-pass")
        print("# " + "".join(f" | {n + ' ms':>15s} {'+-':>7s}" for n in names) + " | ratio")
        print("  " + "".join(f" | {statistics.median(times[n]):15.4f} {max(times[n]) - min(times[n]):7.4f}" for n in names)
              + f" | {statistics.median(times['five layers']) / statistics.median(times['one-pass']):5.3f}", flush=True)


if __name__ == "__main__":
    main()
