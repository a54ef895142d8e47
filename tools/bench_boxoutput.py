#!/usr/bin/env python3
"""BoxOutput alone (boxoutput.hip): B images of device-resident synthetic heads in three regimes (dense / mid / sparse background
bias) at the 7s-576 head sizes (45,630 anchors, 5 classes) and the caltech 480 x 640 ones (12,680 anchors, 2 classes), max_nms_num
2000, in both forms -- image after image (mscnn_boxoutput_fwd_f32) against every image side by side
(mscnn_boxoutput_batch_fwd_f32).  Device time from hip events around `--iters` back-to-back calls after a warm-up, no host
synchronisation inside; workspaces and outputs allocated once.  The forms alternate over `--rounds` rounds (each round starts with
another form); the median round is reported with the spread (max - min over the rounds).  --parent-lib times the per-image op of
another build of libmscnn_hip.so (e.g. the parent commit's) on the same heads, loaded beside this one.  Every form is checked bit for
bit against the one-pass op's output first; --form one_pass / per_image runs that form alone, unchecked (for a kernel trace).
Usage: python tools/bench_boxoutput.py [--iters 100] [--warmup 10] [--rounds 5] [--batches 1,2,4,8,16] [--regimes dense,mid,sparse]
                                      [--shapes 7s-576,caltech] [--parent-lib path/to/libmscnn_hip.so] [--form both|one_pass|per_image]"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mscnn_amd import hipapi  # noqa: E402

DS = [8, 8, 16, 16, 32, 32, 64]
SHAPES = {
    "7s-576": dict(shapes=[(72, 240), (72, 240), (36, 120), (36, 120), (18, 60), (18, 60), (9, 30)], cls=5,
                   field_w=[60, 84, 120, 168, 240, 336, 480], field_h=[60, 84, 120, 168, 240, 336, 480]),
    "caltech": dict(shapes=[(60, 80), (60, 80), (30, 40), (30, 40), (15, 20), (15, 20), (8, 10)], cls=2,
                    field_w=[20, 28, 40, 56, 80, 112, 160], field_h=[40, 56, 80, 112, 160, 224, 320]),
}
REGIMES = {"dense": -8.0, "mid": 2.0, "sparse": 9.0}      # background bias: nearly every anchor / about a half / a few per cent pass fg_thr
GROUP = 32                                                # images per launch group of the one-pass op


def bind(L):
    L.mscnn_last_error.restype = C.c_char_p
    L.mscnn_boxoutput_workspace_bytes.restype = C.c_size_t
    L.mscnn_boxoutput_workspace_bytes.argtypes = [C.c_void_p]
    L.mscnn_boxoutput_max_rows.argtypes = [C.c_void_p]
    L.mscnn_boxoutput_fwd_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_size_t, C.c_void_p]
    return L


def heads_for(gen, geom, B, bias):
    out = []
    for (h, w) in geom["shapes"]:
        t = torch.randn((B, geom["cls"] + 4, h, w), generator=gen, dtype=torch.float32)
        t[:, :geom["cls"]] *= 2.0
        t[:, 0] += bias
        t[:, geom["cls"]:] *= 0.5
        out.append(t.cuda())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", default="1,2,4,8,16")
    ap.add_argument("--regimes", default="dense,mid,sparse")
    ap.add_argument("--shapes", default="7s-576,caltech")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--form", choices=("both", "one_pass", "per_image"), default="both", help="one form alone (for a kernel trace)")
    a = ap.parse_args()

    L = hipapi.lib()
    P = bind(C.CDLL(os.path.abspath(a.parent_lib))) if a.parent_lib and a.form == "both" else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    gen = torch.Generator().manual_seed(1701)
    print(f"# boxoutput.hip, device ms per call from hip events over {a.iters} back-to-back calls after {a.warmup} warm-up, median of "
          f"{a.rounds} rounds with the forms alternating, +- = max - min over the rounds ({torch.cuda.get_device_name()})")
    print("# R = rows of the batch; launches = kernel launches per call (+ 1 memset); ratio = per-image / one-pass")
    names = [n for n in ("per-image", "one-pass") if a.form in ("both", n.replace("-", "_"))] + (["parent per-image"] if P else [])
    print(f"# {'shape':>7s} {'regime':>6s} {'B':>2s} {'R':>6s}" + "".join(f" | {n + ' ms':>19s} {'+-':>6s} {'launches':>8s}" for n in names)
          + (" | ratio" if a.form == "both" else ""))

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

    for shape in a.shapes.split(","):
        geom = SHAPES[shape]
        for regime in a.regimes.split(","):
            for B in [int(b) for b in a.batches.split(",")]:
                heads = heads_for(gen, geom, B, REGIMES[regime])
                d = hipapi.make_boxoutput_desc(geom["shapes"], B, geom["cls"] + 4, geom["field_w"], geom["field_h"], DS)
                ptrs = (C.c_void_p * len(heads))(*[h.data_ptr() for h in heads])
                cap = L.mscnn_boxoutput_max_rows(C.byref(d))

                def make(lib, fwd, wbytes):
                    ws = torch.empty(wbytes, dtype=torch.uint8, device="cuda")
                    out = dict(rois=torch.zeros((cap, 5), dtype=torch.float32, device="cuda"),
                               props=torch.zeros((cap, 6), dtype=torch.float32, device="cuda"),
                               aids=torch.zeros(cap, dtype=torch.int32, device="cuda"), count=torch.zeros(2, dtype=torch.int32, device="cuda"))

                    def run():
                        rc = fwd(C.byref(d), ptrs, out["rois"].data_ptr(), out["props"].data_ptr(), out["aids"].data_ptr(), cap,
                                 out["count"].data_ptr(), ws.data_ptr(), wbytes, st)
                        if rc != 0:
                            raise RuntimeError(lib.mscnn_last_error().decode())
                    return run, out

                forms, outs = {}, {}                         # name -> (what, launches per call), name -> its output buffers
                if a.form != "per_image":
                    fn, outs["one-pass"] = make(L, L.mscnn_boxoutput_batch_fwd_f32, L.mscnn_boxoutput_batch_workspace_bytes(C.byref(d)))
                    forms["one-pass"] = (fn, 4 if B == 1 else 5 * ((B + GROUP - 1) // GROUP))
                for name, lib in ([("per-image", L)] if a.form != "one_pass" else []) + ([("parent per-image", P)] if P else []):
                    fn, outs[name] = make(lib, lib.mscnn_boxoutput_fwd_f32, lib.mscnn_boxoutput_workspace_bytes(C.byref(d)))
                    forms[name] = (fn, 4 * B)
                # The first call of every form.  With one form alone nothing else runs: a kernel trace then holds
                # 1 + rounds x (warmup + iters) calls of that form and no other kernel of this library.  With both, every form is
                # checked bit for bit against the one-pass op.
                for fn, _ in forms.values():
                    fn()
                torch.cuda.synchronize()
                R = int(outs[names[0]]["count"][0])
                if a.form == "both":
                    for name in names:
                        assert torch.equal(outs[name]["count"], outs["one-pass"]["count"]), f"{name} and one-pass differ in (R, real rows)"
                        for k in ("rois", "props", "aids"):
                            assert torch.equal(outs[name][k][:R], outs["one-pass"][k][:R]), f"{name} and one-pass differ in {k}"
                times = {n: [] for n in names}
                for r in range(a.rounds):
                    for k in range(len(names)):
                        n = names[(k + r) % len(names)]
                        times[n].append(timed(forms[n][0]))
                row = f"  {shape:>7s} {regime:>6s} {B:>2d} {R:>6d}"
                for n in names:
                    row += f" | {statistics.median(times[n]):19.4f} {max(times[n]) - min(times[n]):6.4f} {forms[n][1]:>8d}"
                if a.form == "both":
                    row += f" | {statistics.median(times['per-image']) / statistics.median(times['one-pass']):5.2f}"
                print(row, flush=True)


if __name__ == "__main__":
    main()
