"""The crop stage without a GPU: mscnn_net_crop_window -- the host function mscnn_net_crops calls per row; it needs the built library
and no device -- against tests/crops_witness.py (the restatement of include/mscnn_net.h's rule in plain Python numbers) and against
windows written out by hand here; the witness's order, filters and bound on a hand-made pack; the ctypes structs against the header as
a C compiler sees it; the drivers' flag rules through their argument parsers."""
import ctypes as C
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

import crops_witness as cw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 40, 60                                    # the frame of the hand-made rows
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def mnet():
    from mscnn_amd import net
    net.lib()
    return net


def both(mnet, row, org_hw=(H, W), **kw):
    """The C function and the witness on one row; they must agree, and the agreed window is returned."""
    kw = dict(dict(size=(8, 4)), **kw)
    got = mnet.crop_window(kw, row, org_hw)
    want = cw.window(cw.params(**kw), row, org_hw[0], org_hw[1])
    assert got == want, (row, kw, got, want)
    return got


def test_both_functions_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "mscnn_net.h")).read()
    assert "MSCNN_NET_API int mscnn_net_crops(" in text and "MSCNN_NET_API int mscnn_net_crop_window(" in text
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "mscnn_amd", "libmscnn_caffe.so")], capture_output=True, text=True,
                         check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.split()}
    assert {"mscnn_net_crops", "mscnn_net_crop_window"} <= exported


def test_the_ctypes_structs_have_the_c_size_and_offsets(mnet, tmp_path):
    pf = [f for f, _ in mnet.CropsParams._fields_]
    nf = [f for f, _ in mnet.CropInfo._fields_]
    assert pf == ["thr", "context", "fit", "border", "min_size", "out_h", "out_w", "max_crops", "slot", "tracked_only", "mean_bgr"]
    assert nf == ["frame", "slot", "row", "track_id", "x0", "y0", "w", "h"]
    cc = shutil.which("cc") or shutil.which("gcc") or "/opt/rocm/bin/hipcc"
    src = tmp_path / "layout.c"
    prints = ['printf("%d\\n", (int)sizeof(mscnn_crops_params));'] + ['printf("%%d\\n", (int)offsetof(mscnn_crops_params, %s));' % f for f in pf]
    prints += ['printf("%d\\n", (int)sizeof(mscnn_crop_info));'] + ['printf("%%d\\n", (int)offsetof(mscnn_crop_info, %s));' % f for f in nf]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mscnn_net.h"\nint main(void) {\n' + "\n".join(prints) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    lang = ["-x", "c++"] if cc.endswith("hipcc") else []
    r = subprocess.run([cc, "-I" + os.path.join(ROOT, "include"), *lang, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(mnet.CropsParams)] + [getattr(mnet.CropsParams, f).offset for f in pf]
    want += [C.sizeof(mnet.CropInfo)] + [getattr(mnet.CropInfo, f).offset for f in nf]
    assert got == want
    assert got[0] == 64 and got[len(pf) + 1] == 32
    assert mnet.CROP_INFO.itemsize == 32 and list(mnet.CROP_INFO.names) == nf
    assert [mnet.CROP_INFO.fields[f][1] for f in nf] == [getattr(mnet.CropInfo, f).offset for f in nf]
    assert mnet.CROP_BORDERS == cw.BORDERS


def test_hand_made_rows_give_the_windows_written_out_here(mnet):
    # halves round up: x0 + .5 = 2.0 and y0 + .5 = 3.0 exactly
    assert both(mnet, [1.5, 2.5, 4, 3, 0.9]) == (2, 3, 4, 3)
    assert both(mnet, [1.49, 2, 4, 3, 0.9]) == (1, 2, 4, 3)
    # context 1 and 1.5
    assert both(mnet, [10, 10, 8, 4, 0.9]) == (10, 10, 8, 4)
    assert both(mnet, [10, 10, 8, 4, 0.9], context=1.5) == (8, 9, 12, 6)
    assert both(mnet, [10, 10, 5, 3, 0.9], context=1.5) == (9, 9, 7, 5)      # x0 = 8.75, ww = 7.5: L = floor(9.25), R = floor(16.75) - 1
    # fit with size (8, 4), a = 0.5: a narrow box grows its width, a wide one its height
    assert both(mnet, [20, 10, 2, 8, 0.9], fit=True) == (19, 10, 4, 8)
    assert both(mnet, [20, 10, 6, 8, 0.9], fit=True) == (20, 8, 6, 12)
    assert both(mnet, [20, 10, 6, 8, 0.9], fit=False) == (20, 10, 6, 8)
    # all four edges of the 40 x 60 frame: clipped, or shifted inwards at full size
    for row, clip, shift in (([-3, 10, 8, 6, 0.9], (0, 10, 5, 6), (0, 10, 8, 6)), ([55, 10, 8, 6, 0.9], (55, 10, 5, 6), (52, 10, 8, 6)),
                             ([10, -2, 8, 6, 0.9], (10, 0, 8, 4), (10, 0, 8, 6)), ([10, 37, 8, 6, 0.9], (10, 37, 8, 3), (10, 34, 8, 6)),
                             # larger than the frame in one direction (and over the bottom edge in the other), and in both
                             ([-5, 37, 70, 6, 0.9], (0, 37, 60, 3), (0, 34, 60, 6)), ([20, -5, 6, 50, 0.9], (20, 0, 6, 40), (20, 0, 6, 40)),
                             ([-5, -5, 70, 50, 0.9], (0, 0, 60, 40), (0, 0, 60, 40)),
                             # wholly outside: nothing to clip to, but a window that fits is moved inwards
                             ([70, 10, 8, 6, 0.9], None, (52, 10, 8, 6)), ([10, -20, 8, 6, 0.9], None, (10, 0, 8, 6))):
        assert both(mnet, row, border="clip") == clip, row
        assert both(mnet, row, border="shift") == shift, row
    # min_size at the edge of passing, before and after the clip
    assert both(mnet, [10, 10, 5, 3, 0.9], min_size=3) == (10, 10, 5, 3)
    assert both(mnet, [10, 10, 5, 3, 0.9], min_size=4) is None
    assert both(mnet, [57, 10, 5, 5, 0.9], min_size=3) == (57, 10, 3, 5)
    assert both(mnet, [57, 10, 5, 5, 0.9], min_size=4) is None
    assert both(mnet, [57, 10, 5, 5, 0.9], min_size=4, border="shift") == (55, 10, 5, 5)
    # rows that are skipped
    for row in ([NAN, 10, 5, 5, 0.9], [10, NAN, 5, 5, 0.9], [10, 10, NAN, 5, 0.9], [10, 10, 5, NAN, 0.9], [10, 10, 5, 5, NAN],
                [INF, 10, 5, 5, 0.9], [10, -INF, 5, 5, 0.9], [10, 10, INF, 5, 0.9], [10, 10, 5, INF, 0.9], [10, 10, 5, 5, INF],
                [10, 10, -5, 5, 0.9], [10, 10, 5, -5, 0.9], [10, 10, 0, 5, 0.9], [10, 10, 5, 0, 0.9], [10, 10, 0.4, 5, 0.9],
                [0, 0, 2.0 ** 30 + 1, 5, 0.9], [0, 0, 5, 2.0 ** 30 + 1, 0.9], [-2.0 ** 30 - 1, 0, 2.0 ** 31, 5, 0.9], [0, 2.0 ** 30 + 1, 5, 5, 0.9]):
        for border in ("clip", "shift"):
            assert both(mnet, row, border=border) is None, row
    assert both(mnet, [0, 0, 2.0 ** 30, 5, 0.9]) == (0, 0, 60, 5)            # at the bound: cut
    assert both(mnet, [-2.0 ** 30, 0, 2.0 ** 30 + 1, 5, 0.9]) is None
    assert both(mnet, [-2.0 ** 30, 3, 2.0 ** 30, 5, 0.9], context=16.0, min_size=1) is not None      # the largest numbers the rule meets
    # thr equal to the score: cut; just under it: not
    assert both(mnet, [10, 10, 5, 5, 0.3], thr=0.3) == (10, 10, 5, 5)
    assert both(mnet, [10, 10, 5, 5, 0.3 - 1e-12], thr=0.3) is None
    assert both(mnet, [10, 10, 5, 5, -INF], thr=-INF) is None                # (not finite)
    assert both(mnet, [10, 10, 5, 5, -1e300], thr=-INF) == (10, 10, 5, 5)


@pytest.mark.parametrize("fit", [False, True])
@pytest.mark.parametrize("border", ["clip", "shift"])
def test_20000_random_rows_around_and_across_a_37_x_53_frame_equal_the_witness(mnet, fit, border):
    rng = np.random.default_rng(1000 + 2 * int(fit) + (border == "shift"))
    n = 20000
    rows = np.stack([rng.uniform(-30, 80, n), rng.uniform(-30, 60, n), rng.uniform(0.05, 70, n), rng.uniform(0.05, 70, n), rng.uniform(0, 1, n)], axis=1)
    rows[: n // 2, :4] = np.round(rows[: n // 2, :4] * 4) / 4                  # quarters: sums that land exactly on a half
    rows[: n // 2, 2:4] = np.maximum(rows[: n // 2, 2:4], 0.25)
    L = mnet.lib()
    win = (C.c_int * 4)()
    cut = skipped = 0
    for i, size, context, min_size in ((0, (8, 4), 1.0, 1), (1, (5, 7), 1.5, 3), (2, (3, 3), 2.3, 1), (3, (128, 64), 1.0, 6)):
        kw = dict(size=size, thr=0.3, context=context, fit=fit, border=border, min_size=min_size)
        p, wp = mnet.crops_params(**kw), cw.params(**kw)
        for row in rows[i::4]:
            r = (C.c_double * 5)(*row)
            rc = L.mscnn_net_crop_window(C.byref(p), r, 37, 53, win)
            want = cw.window(wp, row, 37, 53)
            assert (tuple(win) if rc == 1 else None) == want and rc in (0, 1), (row.tolist(), kw, rc, tuple(win), want)
            if want:
                cut += 1
                assert want[0] >= 0 and want[1] >= 0 and want[0] + want[2] <= 53 and want[1] + want[3] <= 37 and min(want[2:]) >= min_size
            else:
                skipped += 1
    assert cut > 5000 and skipped > 5000, (cut, skipped)


def test_order_slot_filter_tracked_only_max_crops_and_the_drop_count_on_a_hand_made_pack():
    """Through the witness only: the Net call needs a device (tests/test_gpu_crops.py holds it to this function)."""
    frames = [(40, 60), (30, 50)]
    a = np.array([[10, 10, 8, 6, 0.9], [20, 10, 8, 6, 0.5], [30, 10, 8, 6, 0.2]])      # the last row is under the threshold
    b = np.array([[5, 5, 4, 4, 0.8], [100, 5, 4, 4, 0.7]])                             # the last row lies outside both frames
    segs = [[a, b], [b[:1], a]]
    ids = [[np.array([3, 0, 5]), np.array([0, 7])], [np.array([9]), np.array([0, 4, 4])]]
    p = cw.params(size=(8, 4), thr=0.3, max_crops=100)
    got, dropped = cw.crops(frames, segs, p, ids)
    assert dropped == 0 and got == [(0, 0, 0, 3, 10, 10, 8, 6), (0, 0, 1, 0, 20, 10, 8, 6), (0, 1, 0, 0, 5, 5, 4, 4), (1, 0, 0, 9, 5, 5, 4, 4),
                                    (1, 1, 0, 0, 10, 10, 8, 6), (1, 1, 1, 4, 20, 10, 8, 6)]
    assert cw.crops(frames, segs, p, None) == ([g[:3] + (0,) + g[4:] for g in got], 0)
    assert cw.crops(frames, segs, dict(p, slot=1), ids) == ([g for g in got if g[1] == 1], 0)
    assert cw.crops(frames, segs, dict(p, tracked_only=1), ids) == ([g for g in got if g[3] > 0], 0)
    assert cw.crops(frames, segs, dict(p, max_crops=4), ids) == (got[:4], 2)
    assert cw.crops(frames, segs, dict(p, max_crops=1, slot=1, tracked_only=1), ids) == ([got[5]], 0)
    assert cw.crops(frames, segs, dict(p, max_crops=1, slot=0, tracked_only=1), ids) == ([got[0]], 1)      # the filters apply before counting
    assert cw.crops(frames, segs, dict(p, thr=0.95), ids) == ([], 0)
    assert cw.crops(frames, [[None, b], [b[:1], np.zeros((0, 5))]], p, None)[0] == [(0, 1, 0, 0, 5, 5, 4, 4), (1, 0, 0, 0, 5, 5, 4, 4)]


def test_every_refusal_of_crop_window_names_its_value(mnet):
    ok = dict(size=(8, 4))
    row = [10, 10, 5, 5, 0.9]
    for kw, text in ((dict(thr=NAN), "crop_window: thr is NaN"), (dict(context=0.99), "context 0.99 is outside [1, 16]"),
                     (dict(context=16.5), "context 16.5 is outside [1, 16]"), (dict(context=NAN), "context nan is outside [1, 16]"),
                     (dict(fit=2), "fit 2 is neither 0 nor 1"), (dict(fit=-1), "fit -1 is neither 0 nor 1"),
                     (dict(border=2), "border 2 is neither 0 (clip) nor 1 (shift)"), (dict(border=-1), "border -1 is neither 0 (clip) nor 1 (shift)"),
                     (dict(min_size=0), "min_size 0 is below 1"), (dict(size=(0, 4)), "out_h 0 is outside [1, 1024]"),
                     (dict(size=(1025, 4)), "out_h 1025 is outside [1, 1024]"), (dict(size=(8, 0)), "out_w 0 is outside [1, 1024]"),
                     (dict(size=(8, 1025)), "out_w 1025 is outside [1, 1024]"), (dict(max_crops=0), "max_crops 0 is below 1"),
                     (dict(slot=-2), "slot -2 is below -1"), (dict(tracked_only=2), "tracked_only 2 is neither 0 nor 1"),
                     (dict(mean=(0, INF, 0)), "mean_bgr[1] inf is not finite"), (dict(mean=(0, 0, NAN)), "mean_bgr[2] nan is not finite")):
        with pytest.raises(mnet.NetError) as e:
            mnet.crop_window(dict(ok, **kw), row, (H, W))
        assert text in str(e.value) and str(e.value).startswith("crop_window: "), (kw, str(e.value))
    for hw, text in (((0, 60), "the frame is 0 x 60"), ((40, -1), "the frame is 40 x -1"), ((2 ** 30 + 1, 60), "the frame is 1073741825 x 60")):
        with pytest.raises(mnet.NetError) as e:
            mnet.crop_window(ok, row, hw)
        assert text in str(e.value)
    L = mnet.lib()
    p = mnet.crops_params(**ok)
    assert L.mscnn_net_crop_window(None, (C.c_double * 5)(*row), H, W, (C.c_int * 4)()) < 0 and b"null pointer" in L.mscnn_net_last_error()
    assert L.mscnn_net_crop_window(C.byref(p), None, H, W, (C.c_int * 4)()) < 0 and L.mscnn_net_crop_window(C.byref(p), (C.c_double * 5)(*row), H, W, None) < 0
    with pytest.raises(mnet.NetError, match="border 'wrap' is none of"):
        mnet.crop_window(dict(ok, border="wrap"), row, (H, W))
    assert mnet.crop_window(dict(ok, size=(1024, 1024), context=16.0, slot=5, tracked_only=True, mean=(104, 117, 123)), row, (2 ** 30, 2 ** 30)) is not None


def test_a_net_without_a_device_refuses_the_call_and_the_wrapper_names_bad_arguments(mnet):
    from mscnn_amd import zoo
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=96, width=320, max_nms_num=200), device=-1)
    frames = [np.zeros((12, 20, 3), np.uint8)] * 2
    out = np.full((3, 3, 8, 4), -7.5, np.float32)
    with pytest.raises(mnet.NetError, match=r"crops: the net was built with device -1 \(graph only\)"):
        n.crops(frames, size=(8, 4), out=out)
    with pytest.raises(mnet.NetError, match=r"crops: the net was built with device -1"):
        n.crops(frames, size=(8, 4))
    assert (out == -7.5).all()
    for kw, text in ((dict(out=np.zeros((3, 3, 8, 5), np.float32)), r"out is not a contiguous float32 buffer of shape \[>= 3, 3, 8, 4\]"),
                     (dict(out=out, max_crops=4), r"shape \[>= 4, 3, 8, 4\]"), (dict(out=out.astype(np.float64)), "out is not a contiguous float32"),
                     (dict(border="wrap"), "border 'wrap' is none of"), (dict(mean=(1, 2)), "mean holds 2 values")):
        with pytest.raises(mnet.NetError, match=text):
            n.crops(frames, size=(8, 4), **kw)
    with pytest.raises(mnet.NetError, match="crops: frame 1 is not a uint8"):
        n.crops([frames[0], np.zeros((12, 20), np.uint8)], size=(8, 4))


def driver(tool, monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(ROOT, "tools"))      # (run_cascademscnn imports run_mscnn_detection, as a script's directory gives it)
    spec = importlib.util.spec_from_file_location(tool[:-3] + "_crops_under_test", os.path.join(ROOT, "tools", tool))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    return drv


@pytest.mark.parametrize("tool,model", [("run_mscnn_detection.py", "kitti_car/mscnn-7s-576"), ("run_cascademscnn.py", "kitti_car/cascade-mscnn-7s-576-2x")])
def test_both_drivers_refuse_the_flag_combinations(monkeypatch, capsys, tool, model):
    drv = driver(tool, monkeypatch)
    base = ["--model", model, "--synthetic", "1"]
    belong = "belong to --crops-out"
    cases = [(["--crop-size", "64x32"], belong), (["--crop-thr", "0.5"], belong), (["--crop-context", "1.5"], belong), (["--crop-fit"], belong),
             (["--crop-border", "shift"], belong), (["--crop-min", "8"], belong), (["--crop-tracked"], belong),
             (["--crops-out", "x", "--crop-tracked"], "it needs --track"),
             (["--crops-out", "x", "--crop-size", "64"], "--crop-size '64' is not HxW"), (["--crops-out", "x", "--crop-size", "0x64"], "is not HxW"),
             (["--crops-out", "x", "--crop-size", "64x1025"], "inside 1 .. 1024"),
             (["--crops-out", "x", "--crop-context", "0.5"], "--crop-context 0.5: the factor must lie inside [1, 16]"),
             (["--crops-out", "x", "--crop-context", "nan"], "must lie inside [1, 16]"), (["--crops-out", "x", "--crop-thr", "nan"], "--crop-thr nan"),
             (["--crops-out", "x", "--crop-min", "0"], "--crop-min 0: must be >= 1")]
    if tool == "run_mscnn_detection.py":         # where --render-out is refused, for the same reason
        cases += [(["--crops-out", "x", "--proposals-only", "--proposals-out", "p"], "--crops-out cuts the detections"),
                  (["--crops-out", "x", "--rois-in", "r.txt"], "--crops-out cuts the detections")]
    for extra, text in cases:
        with pytest.raises(SystemExit):
            drv.parse_args(base + extra)
        assert text in capsys.readouterr().err, extra
    a = drv.parse_args(base + ["--crops-out", "x"])
    assert a.crop_size == (128, 64) and a.crop_context == 1.0 and not a.crop_fit and a.crop_border == "clip" and a.crop_min == 1 and not a.crop_tracked
    a = drv.parse_args(base + ["--crops-out", "x", "--track", "--crop-tracked", "--crop-size", "96x48", "--crop-thr", "0.6", "--crop-context", "1.5",
                               "--crop-fit", "--crop-border", "shift", "--crop-min", "8", "--batch", "3", "--streams", "3", "--render-out", "y",
                               "--show-thr", "0.4"])
    assert a.crop_size == (96, 48) and a.crop_thr == 0.6 and a.crop_tracked and a.render_out == "y"
    a = drv.parse_args(base + ["--crops-out", "x", "--flip", "--vote"])
    assert a.crops_out == "x" and a.flip


def test_the_drivers_pixel_rule(monkeypatch):
    drv = driver("run_mscnn_detection.py", monkeypatch)
    patch = np.zeros((3, 1, 6), np.float32)
    patch[0, 0] = [-3.2, -0.5, 0.49, 0.5, 254.5, 300.0]      # plane B
    patch[1, 0] = 7
    patch[2, 0] = [1.5, 2.5, 3.4999, 254.49, 255.0, 1e9]     # plane R
    got = drv.patch_to_rgb_u8(patch)
    assert got.shape == (1, 6, 3) and got.dtype == np.uint8
    assert got[0, :, 2].tolist() == [0, 0, 0, 1, 255, 255] and got[0, :, 1].tolist() == [7] * 6 and got[0, :, 0].tolist() == [2, 3, 3, 254, 255, 255]
