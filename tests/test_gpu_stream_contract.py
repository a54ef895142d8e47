"""The STREAM CONTRACT of the C ABI (include/mscnn_hip.h), op family by op family, and two streams in flight from one host thread.

Ordering and asynchrony: every case of tests/stream_cases.py runs through tests/streams.py's gated runner -- the op is enqueued on
a non-blocking side stream behind a gate while its device inputs still hold a stale draw, the real inputs arrive by copies on that
stream, the inputs are overwritten and the workspaces scribbled behind the call, and the outputs must be bit-identical to a
default-stream run that was first held to the op's own bar against the oracle.  `busy` (the stream still had the gate in front of
it when the call returned) proves both that the call did not wait and that the gate was long enough.  No tolerance is introduced.

Concurrency: two side streams, a gate of equal length on each, then four alternating calls per stream on different inputs and
different outputs; every output must be bit-identical to its serial result.  The InnerProduct cases are the regression test of
the stream-K slab buffer of gemm.hip, which is kept per (thread, device, stream): with one buffer per (thread, device) one call's
fix-up kernel could read slabs that the other stream's main kernel had overwritten.  The interleaving can not be forced, so this
test could pass on the old code on a given day; the hazard was certain from the code.  No case here uses a persistent-grid kernel
that waits inside the kernel (no wgemm plan with split tiles, no inner_product_wg): co-residency of their workgroups is a stated
precondition of those kernels, and on a device shared between two streams they may legitimately raise a hand-off event.

Gate lengths are measured, not fixed: ten times the host time of the case's own enqueue block (tests/streams.py), never under
5 ms; each case prints its figures (`[stream] ...`, pytest -s).  On an MI355X the enqueue blocks took 0.03 - 0.5 ms, so the 5 ms
floor was the gate of nearly every case; in each of two runs one conv case (a different one) took 5.5 and 5.7 ms to enqueue and
got a gate of 55 and 57 ms.  Largest enqueue 5.71 ms, largest gate asked 57.1 ms (measured 57.2 ms); the gates came out within
0.02 ms of what was asked; every case was busy.

One output is not compared bit for bit: mscnn_sum_squares_f32 adds per-wave partial sums with f64 atomics, so its last bits change
from run to run on ANY stream (Case.unordered); its side-stream result is held to the op's own 1e-9 bar instead."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import stream_cases, streams  # noqa: E402


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X: torch.cuda.is_available() is False")
    from mscnn_amd import hipapi
    hipapi.lib()
    return hipapi


@pytest.fixture(scope="module")
def side():
    return torch.cuda.Stream()


@pytest.mark.parametrize("case", stream_cases.CASES, ids=lambda c: c.name)
def test_gated(hip, orc, side, case):
    streams.run_gated(case, hip, orc, side)


# ================================================================================================ two streams in flight
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def run_two_streams(hip, lanes, name):
    """lanes: two lists of closures, one list per stream; a closure enqueues one call on the current stream and returns its output
    tensors (its own).  Serial results first, then an ungated interleaved pass (first-call work, allocator, the enqueue time), then
    the gated interleaved pass."""
    assert len(lanes) == 2 and len(lanes[0]) == len(lanes[1])
    handoff = hip.wgemm_handoff_event()
    ref = []
    for lane in lanes:
        for f in lane:
            outs = f()
            torch.cuda.synchronize()
            ref.append([o.cpu().numpy().copy() for o in outs])
    s = [torch.cuda.Stream(), torch.cuda.Stream()]
    pinned = [[torch.empty(r.shape, dtype=torch.from_numpy(r).dtype, pin_memory=True) for r in rr] for rr in ref]
    n = len(lanes[0])

    def interleaved(gate_ms):
        torch.cuda.synchronize()
        for k in (0, 1):
            with torch.cuda.stream(s[k]):
                if gate_ms:
                    streams.gate(s[k], gate_ms)
        t0 = time.perf_counter()
        keep = []
        for i in range(n):
            for k in (0, 1):
                with torch.cuda.stream(s[k]):
                    outs = lanes[k][i]()
                    for h, o in zip(pinned[k * n + i], outs):
                        h.copy_(o, non_blocking=True)
                    keep.append(outs)
        busy = [not s[0].query(), not s[1].query()]
        ms = (time.perf_counter() - t0) * 1e3
        s[0].synchronize()
        s[1].synchronize()
        return busy, ms, [[h.numpy().copy() for h in hh] for hh in pinned]

    streams.calibrate(s[0])
    interleaved(0)
    _, enqueue_ms, got = interleaved(0)
    gate_ms = max(streams.GATE_FACTOR * enqueue_ms, streams.MIN_GATE_MS)
    busy, _, got = interleaved(gate_ms)
    print(f"[stream] two streams, {name}: enqueue {enqueue_ms:.3f} ms, gate {gate_ms:.2f} ms per stream, busy {busy}")
    assert all(busy), f"{name}: a stream was idle when the last call returned (gate {gate_ms:.2f} ms, enqueue {enqueue_ms:.3f} ms)"
    for j, (g, r) in enumerate(zip(got, ref)):
        for a, b in zip(g, r):
            assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), f"{name}: call {j % n} of stream {j // n} differs from its serial result"
    assert hip.wgemm_handoff_event() == handoff
    return ref


@pytest.mark.parametrize("M,N,K,f16", [(700, 2048, 3200, False), (700, 2048, 3200, True), (676, 8, 4096, False)],
                         ids=["f32_mfma_streamk", "f16_mfma_streamk", "f32_rowwise"])
def test_two_streams_inner_product(hip, M, N, K, f16):
    """(700, 2048, 3200): the MFMA stream-K path -- tiles are split between workgroups, so the library's slabs carry partial sums;
    (676, 8, 4096): the row-wise kernel, a case without library state."""
    from tests.test_gpu_buffer_contract import _ip_data
    L = hip.lib()
    lanes, first = [], None
    for k in (0, 1):
        x0, w, b, ref0 = _ip_data(M, N, K, 31 + k, exact16=f16)
        first = first or (x0, w, b, ref0)
        wd, bd = dev(w), dev(b)
        if f16:
            w16 = torch.empty(N * K, dtype=torch.float16, device="cuda")
            hip._check(L.mscnn_inner_product_pack_f16(hip._dev(wd), hip._dev(w16), N, K, hip._stream()))
        lane = []
        for i in range(4):
            xd = dev(np.roll(x0, 7 * i + 1, axis=0) * np.float32(1 + i)) if i else dev(x0)      # (call 0 is the one held to the float64 bar)
            if f16:
                def call(xd=xd, w16=w16, bd=bd):
                    y = torch.empty((M, N), dtype=torch.float32, device="cuda")
                    hip._check(L.mscnn_inner_product_fwd_f16(hip._dev(xd), hip._dev(w16), hip._dev(bd), hip._dev(y), M, N, K, 0, hip._stream()))
                    return [y]
            else:
                def call(xd=xd, wd=wd, bd=bd):
                    return [hip.inner_product(xd, wd, bd)]
            lane.append(call)
        lanes.append(lane)
    torch.cuda.synchronize()
    ref = run_two_streams(hip, lanes, f"inner_product M={M} N={N} K={K} f16={f16}")
    err = np.abs(ref[0][0] - first[3]) / np.maximum(1.0, np.abs(first[3]))      # the serial result itself: the suite's bar for the op
    assert err.max() <= 1e-4, err.max()


def test_two_streams_conv_igemm_streamk(hip, orc):
    """Two plans of the igemm stream-K class (slabs in the plan's own workspace), each with its own workspace."""
    N, Cin, H, W, Cout = 1, 24, 36, 120, 256
    lanes, first = [], None
    for k in (0, 1):
        rng = np.random.default_rng(50 + k)
        w = (rng.standard_normal((Cout, Cin, 3, 3)) * np.sqrt(2.0 / (Cin * 9))).astype(np.float32)
        b = rng.standard_normal(Cout).astype(np.float32)
        plan = hip.ConvPlan(N, Cin, H, W, Cout, 3, 3, (1, 1), relu=True, algo=hip.ALGO_DIRECT)
        assert plan.kernel.startswith("igemm_") and plan.plan_class()["ig_sched"] == 3 and plan.ws is not None, plan.kernel
        plan.pack(dev(w))
        bd = dev(b)
        xs = [rng.standard_normal((N, Cin, H, W)).astype(np.float32) for _ in range(4)]
        first = first or (xs[0], w, b)
        lanes.append([(lambda xd=dev(x), plan=plan, bd=bd: [plan.forward(xd, bd)]) for x in xs])
    torch.cuda.synchronize()
    ref = run_two_streams(hip, lanes, "conv igemm stream-K")
    want = orc.relu(orc.conv2d(first[0], first[1], first[2], (1, 1)))
    err = np.abs(ref[0][0] - want) / np.maximum(1.0, np.abs(want))
    assert err.max() <= 1e-4, err.max()


def test_two_streams_boxoutput(hip, orc):
    """Two BoxOutput layers, each with its own workspace and output buffers (copied out behind each call, on the call's stream)."""
    from tests.test_gpu_buffer_contract import KITTI_HEADS, _heads
    kw = stream_cases.BO_KW
    lanes, first = [], None
    for k in (0, 1):
        d = hip.make_boxoutput_desc(KITTI_HEADS["shapes"], 1, 9, KITTI_HEADS["field"], KITTI_HEADS["field"], KITTI_HEADS["ds"], **kw)
        layer = hip.BoxOutput(d)
        lane = []
        for i in range(4):
            heads = _heads(np.random.default_rng(900 + 10 * k + i), KITTI_HEADS["shapes"], bg_bias=-8.0)
            first = first or heads
            hd = [dev(h) for h in heads]

            def call(layer=layer, hd=hd):
                for t in (layer.rois, layer.props, layer.aids):      # rows past the count are not the op's to write: zeros in every run
                    t.zero_()
                layer.forward_async(hd)
                return [layer.count.clone(), layer.rois.clone(), layer.props.clone(), layer.aids.clone()]
            lane.append(call)
        lanes.append(lane)
    torch.cuda.synchronize()
    ref = run_two_streams(hip, lanes, "boxoutput")
    rois_r, props_r, _, nreal_r, aids_r = orc.boxoutput(first, KITTI_HEADS["field"], KITTI_HEADS["field"], KITTI_HEADS["ds"], with_anchor_ids=True, **kw)
    R, nreal = ref[0][0].tolist()
    assert nreal == nreal_r and np.array_equal(ref[0][1][:R], rois_r) and np.array_equal(ref[0][2][:R], props_r) and np.array_equal(ref[0][3][:R], aids_r)


def test_two_streams_detections_multi(hip, orc):
    """Two detections_multi states, each with its own workspace; every call writes a pack of its own."""
    lanes, first = [], None
    for k in (0, 1):
        state = stream_cases.multi_state(hip, False)
        lane = []
        for i in range(4):
            _, inp = stream_cases.multi_inputs(70 + 10 * k + i, False)
            first = first or inp
            bufs = {n: dev(a) for n, a in inp.items()}
            lane.append(lambda state=state, bufs=bufs: stream_cases.multi_run(hip, state, bufs, False))
        lanes.append(lane)
    torch.cuda.synchronize()
    ref = run_two_streams(hip, lanes, "detections_multi")
    stream_cases.multi_check(hip, orc, first, ref[0][0], False)
