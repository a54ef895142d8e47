#!/usr/bin/env python3
"""Frame pre-processing alone (preprocess.hip): B device-resident uint8 frames of mixed KITTI sizes (375x1242, 370x1224, 374x1238,
376x1241, cycled) to the net's input, in both forms -- a loop of B single-frame ops (mscnn_preprocess_u8_f32) against one batched op
(mscnn_preprocess_batch_u8_f32).  Device time from hip events around `--iters` back-to-back repetitions after a warm-up, no host
synchronisation inside; workspaces and outputs allocated once.  The forms alternate over `--rounds` rounds (each round starts with
another form); the median round is reported.  --parent-lib times the single-frame loop of another build of
libmscnn_hip.so (e.g. the parent commit's) on the same frames, loaded beside this one.  Every form is checked bit for bit against
the batched op's output first.
Usage: python tools/bench_preprocess.py [--iters 200] [--warmup 20] [--rounds 5] [--parent-lib path/to/libmscnn_hip.so]
                                       [--form both|batch]"""
import argparse
import statistics
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mscnn_amd import hipapi  # noqa: E402

SIZES = [(375, 1242), (370, 1224), (374, 1238), (376, 1241)]
TARGETS = [(576, 1920), (480, 640)]
CAP = 32    # frames per launch pair of the batched op


def bind(L):
    L.mscnn_preprocess_workspace_bytes.restype = C.c_size_t
    L.mscnn_preprocess_workspace_bytes.argtypes = [C.c_int] * 4
    L.mscnn_preprocess_u8_f32.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                          C.c_void_p]
    L.mscnn_last_error.restype = C.c_char_p
    return L


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--form", choices=("both", "batch"), default="both", help="batch: the batched op alone (for a kernel trace)")
    a = ap.parse_args()

    L = bind(hipapi.lib())
    L.mscnn_preprocess_batch_workspace_bytes.restype = C.c_size_t
    L.mscnn_preprocess_batch_workspace_bytes.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    P = bind(C.CDLL(os.path.abspath(a.parent_lib))) if a.parent_lib else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    mean = (C.c_float * 3)(104.0, 117.0, 123.0)
    gen = torch.Generator().manual_seed(1701)
    print(f"# preprocess.hip, device ms from hip events over {a.iters} repetitions after {a.warmup} warm-up, median of {a.rounds} rounds "
          f"with the forms alternating ({torch.cuda.get_device_name()})")
    print(f"# frames cycle through {', '.join(f'{h}x{w}' for h, w in SIZES)}; launches = kernel launches per batch")
    hdr = f"# {'target':>9s} {'B':>2s} | {'loop ms/batch':>14s} {'ms/frame':>8s} {'launches':>8s} | {'batch ms/batch':>14s} {'ms/frame':>8s} {'launches':>8s}"
    print(hdr + (f" | {'parent loop ms/batch':>20s} {'ms/frame':>8s}" if P else ""))

    def check(rc, lib):
        if rc != 0:
            raise RuntimeError(lib.mscnn_last_error().decode())

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters

    for H, W in TARGETS:
        for B in [int(b) for b in a.batches.split(",")]:
            orgs = [SIZES[b % len(SIZES)] for b in range(B)]
            frames = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=gen).cuda() for h, w in orgs]
            oh = (C.c_int * B)(*[h for h, _ in orgs])
            ow = (C.c_int * B)(*[w for _, w in orgs])
            ptrs = (C.c_void_p * B)(*[f.data_ptr() for f in frames])
            out_b = torch.empty((B, 3, H, W), dtype=torch.float32, device="cuda")
            wb = L.mscnn_preprocess_batch_workspace_bytes(B, oh, ow, H, W)
            ws_b = torch.empty(wb, dtype=torch.uint8, device="cuda")

            def batch():
                check(L.mscnn_preprocess_batch_u8_f32(ptrs, oh, ow, B, C.c_void_p(out_b.data_ptr()), H, W, mean, C.c_void_p(ws_b.data_ptr()),
                                                      C.c_size_t(wb), st), L)

            out_l = torch.empty_like(out_b)
            w1 = max(L.mscnn_preprocess_workspace_bytes(h, w, H, W) for h, w in orgs)
            ws_1 = torch.empty(w1, dtype=torch.uint8, device="cuda")      # one scratch for the loop: the frames run in stream order

            def loop(lib):
                for b in range(B):
                    check(lib.mscnn_preprocess_u8_f32(C.c_void_p(frames[b].data_ptr()), orgs[b][0], orgs[b][1],
                                                      C.c_void_p(out_l[b].data_ptr()), H, W, mean, C.c_void_p(ws_1.data_ptr()), C.c_size_t(w1), st), lib)

            batch()
            forms = [(batch, 2 * ((B + CAP - 1) // CAP))]          # (what, launches per batch; None: not this library's)
            if a.form == "both":
                for lib in [L] + ([P] if P else []):
                    out_l.fill_(float("nan"))
                    loop(lib)
                    torch.cuda.synchronize()
                    assert torch.equal(out_l, out_b), "single-frame loop and batched op differ"
                forms.insert(0, (lambda: loop(L), 2 * B))
                if P:
                    forms.append((lambda: loop(P), None))
            times = [[] for _ in forms]
            for r in range(a.rounds):
                for k in range(len(forms)):
                    f = (k + r) % len(forms)
                    times[f].append(timed(forms[f][0]))
            row = f"  {H:>4d}x{W:<4d} {B:>2d}"
            for ts, (_, n) in zip(times, forms):
                t = statistics.median(ts)
                row += f" | {t:{14 if n is not None else 20}.4f} {t / B:8.4f}" + (f" {n:>8d}" if n is not None else "")
            print(row, flush=True)


if __name__ == "__main__":
    main()
