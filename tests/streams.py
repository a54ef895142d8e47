"""A gate and a runner for the stream-contract tests (tests/test_gpu_stream_contract.py, tests/test_gpu_net_streams.py).

    from tests import streams

gate(stream, ms) enqueues device work of a known length on `stream`: torch.cuda._sleep where the installed torch has it, else a
chain of torch matmuls.  Either is calibrated once per process with events around the gate itself.  It is plain device work that
always ends; nothing on the device waits for the host.

run_gated(case, hip, orc, side) holds one Case to the ordering and asynchrony rules of the STREAM CONTRACT (include/mscnn_hip.h):

  1. the case runs on the default stream with full synchronisation; the result is `ref`, and case.check holds it to the op's
     existing bar against the oracle or a float64 reference -- what follows compares with a checked result;
  2. two ungated runs on the side stream: the first warms torch's allocator for that stream and the library's first-call work,
     the second measures the host time of the enqueue block (input copies, the op, the overwrites, the D2H enqueue);
  3. the gated run.  The device inputs hold a STALE draw (another valid input of the same shapes).  On the side stream: the gate,
     sized ten times the measured enqueue time (and no shorter than MIN_GATE_MS); device-to-device copies of the real inputs over
     the stale ones; the op; busy = not side.query() the moment it returns; every input overwritten with a THIRD valid draw, every
     workspace the case names scribbled; the D2H copies of the outputs into pinned memory; side.synchronize() -- never a device
     synchronisation;
  4. busy must hold -- the call did not wait, and it was enqueued while its inputs were still stale, so the gate was long enough:
     one that was too short fails the test --, and the outputs must be bit-identical to `ref`.

What that catches: a launch, memset or copy on the NULL stream or a private one (it runs in front of the gate, on stale inputs or
on an output that is overwritten later); a host-side read of device memory and an internal wait (busy); an input consumed after
the call's place in the stream (the third draw).  The default stream stays idle during the gated run; torch's side streams are
non-blocking, so the legacy stream does not order itself against them.

A stale or third draw is never garbage: ROI lists, counts, indices and packs are valid in every draw, so an op that reads early or
late computes a valid but different answer."""
import time

import numpy as np
import torch

MIN_GATE_MS = 5.0
GATE_FACTOR = 10.0
_rate = {}          # "sleep": cycles per ms, "matmul": products per ms
_mm = {}


def _gate_kind():
    return "sleep" if hasattr(torch.cuda, "_sleep") else "matmul"


def _enqueue(kind, units):
    if kind == "sleep":
        torch.cuda._sleep(int(units))
    else:
        a = _mm.setdefault("a", torch.full((1024, 1024), 1.0 / 1024, dtype=torch.float32, device="cuda"))
        for _ in range(max(int(units), 1)):
            a = a @ _mm["a"]
        _mm["last"] = a


def _timed(stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record(stream)
        fn()
        e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def calibrate(stream):
    """Units of gate work per millisecond on this device, measured with events around the gate itself."""
    kind = _gate_kind()
    if kind not in _rate:
        probe = 20_000_000 if kind == "sleep" else 64
        _timed(stream, lambda: _enqueue(kind, probe))                 # the first launch of the kernel
        ms = min(_timed(stream, lambda: _enqueue(kind, probe)) for _ in range(2))
        _rate[kind] = probe / max(ms, 1e-3)
    return _rate[kind]


def gate(stream, ms):
    """Enqueue about `ms` milliseconds of device work on `stream` (the current stream must be `stream`)."""
    kind = _gate_kind()
    _enqueue(kind, max(calibrate(stream) * ms, 1))


class Case:
    """One gated case.
      name        the test id
      abi         the C-ABI functions with a `void* stream` parameter that run() calls (tests/test_stream_cases_cpu.py)
      draw(seed)  -> {name: numpy array}: one valid set of inputs; the shapes do not depend on the seed
      setup(hip)  -> state that lives across the runs (plans, workspaces, descriptors), or None
      run(hip, state, bufs) -> list of device tensors: the op on the device buffers `bufs` (same keys as draw), on the current stream,
                  returning without a read of device memory
      check(orc, inputs, outs)   the op's existing bar: outs (numpy, in run's order) against the oracle / float64 reference
      workspaces(state) -> tensors to scribble behind the call
      busy        False where the call is allowed to wait, with `why` naming the line that does"""

    def __init__(self, name, abi, draw, run, check, setup=None, workspaces=None, busy=True, why=None, seed=1701, unordered=()):
        self.name, self.abi, self.draw, self.run, self.check = name, tuple(abi), draw, run, check
        self.setup, self.workspaces, self.busy, self.why, self.seed = setup, workspaces, busy, why, seed
        # unordered: indices of outputs that are sums of floating-point atomics, whose order the hardware picks: two runs on ONE
        # stream already differ in the last bits.  They are not compared bit for bit; instead the side-stream outputs as a whole go
        # through check(), the op's own bar -- far tighter than the distance between two draws.
        self.unordered = tuple(unordered)
        assert busy or why, name

    def __repr__(self):
        return self.name


def scribble(t, byte=0x5A):
    t.view(-1).view(torch.uint8).fill_(byte)


def _upload(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}


REPORT = []          # (case name, enqueue ms, gate ms asked, gate ms measured): printed by the GPU file, largest go into its docstring


def run_gated(case, hip, orc, side):
    real, stale, third = (case.draw(case.seed + i) for i in range(3))
    for k in real:
        assert real[k].shape == stale[k].shape == third[k].shape and real[k].dtype == stale[k].dtype == third[k].dtype, (case, k)
    assert any(not np.array_equal(real[k], stale[k]) for k in real) and any(not np.array_equal(real[k], third[k]) for k in real)
    real_d, stale_d, third_d = _upload(real), _upload(stale), _upload(third)
    bufs = {k: v.clone() for k, v in real_d.items()}
    state = case.setup(hip) if case.setup else None
    handoff = hip.wgemm_handoff_event()

    # 1. the default stream, fully synchronised, against the op's own bar
    outs = case.run(hip, state, bufs)
    torch.cuda.synchronize()
    ref = [o.cpu().numpy().copy() for o in outs]
    case.check(orc, real, ref)
    pinned = [torch.empty(tuple(o.shape), dtype=o.dtype, pin_memory=True) for o in outs]
    del outs

    def block(gate_ms):
        for k in bufs:
            bufs[k].copy_(stale_d[k])
        for h in pinned:
            h.view(-1).view(torch.uint8).fill_(0xEE)
        torch.cuda.synchronize()
        g0, g1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(side):
            if gate_ms:
                g0.record(side)
                gate(side, gate_ms)
                g1.record(side)
            t0 = time.perf_counter()
            for k in bufs:
                bufs[k].copy_(real_d[k], non_blocking=True)
            outs = case.run(hip, state, bufs)
            busy = not side.query()
            for k in bufs:
                bufs[k].copy_(third_d[k], non_blocking=True)
            for w in (case.workspaces(state) if case.workspaces else []):
                if w is not None:
                    scribble(w)
            for h, o in zip(pinned, outs):
                h.copy_(o, non_blocking=True)
            t1 = time.perf_counter()
            side.synchronize()
        got = [h.numpy().copy() for h in pinned]
        return busy, got, (t1 - t0) * 1e3, (g0.elapsed_time(g1) if gate_ms else 0.0)

    # 2. ungated on the side stream: warm, then measure the enqueue block
    calibrate(side)
    block(0)
    _, got, enqueue_ms, _ = block(0)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert i in case.unordered or (g.shape == r.shape and np.array_equal(g.view(np.uint8), r.view(np.uint8))), \
            f"{case}: output {i} of the ungated side-stream run differs"

    # 3. gated
    gate_ms = max(GATE_FACTOR * enqueue_ms, MIN_GATE_MS)
    busy, got, _, gate_measured = block(gate_ms)
    REPORT.append((case.name, enqueue_ms, gate_ms, gate_measured))
    print(f"[stream] {case.name}: enqueue {enqueue_ms:.3f} ms, gate asked {gate_ms:.2f} ms, measured {gate_measured:.2f} ms, busy {busy}")

    # 4.
    if case.busy:
        assert busy, (f"{case}: the side stream was idle when the call returned -- the call waited for the device, or the gate "
                      f"({gate_measured:.2f} ms for an enqueue block of {enqueue_ms:.3f} ms) was too short")
    for i, (g, r) in enumerate(zip(got, ref)):
        assert i in case.unordered or (g.shape == r.shape and np.array_equal(g.view(np.uint8), r.view(np.uint8))), \
            f"{case}: output {i} of the gated side-stream run differs from the default-stream run"
    if case.unordered:
        case.check(orc, real, got)
    assert hip.wgemm_handoff_event() == handoff, f"{case}: a stream-K hand-off event was raised"
    return ref
