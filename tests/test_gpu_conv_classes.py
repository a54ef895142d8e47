"""Every convolution plan class the deploy nets select (tests/conv_classes.py: CASES, one small row per class of the census) against
torch.nn.functional.conv2d in float64 on the CPU -- never against another plan of this library.

Inputs: x post-ReLU at unit scale, He-scaled weights, random bias, all seeded; every channel and tap distinct.  Bars: the fp32 families
and the split-fp16 ones (f16x3: "not a reduced-precision mode", test_gpu_ops.py::test_conv_winograd_x3 / test_conv_direct_x3) meet
|a - b| <= 1e-4 * max(1, |b|), the bar of test_gpu_ops.py; the fp16-operand kernels get operands a fp16 MFMA input represents exactly
and meet the same 1e-4, as test_gpu_ops.py::test_conv_f16_planes does (the products then fit fp32, so a layout or indexing error
cannot hide in rounding noise).  Further: the pooled epilogue is bit-identical to pooling y, the pooled-only call too, the published
max |y| is the tensor's, and a second forward of the same plan at another N of the same class still meets the bar."""
import numpy as np
import pytest

import conv_classes as cc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL = 1e-4


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X: torch.cuda.is_available() is False")
    from mscnn_amd import hipapi
    hipapi.lib()
    return hipapi


def _fp16_exact(a):
    return a.astype(np.float16).astype(np.float32)


def _inputs(row, n_images):
    d = row["desc"]
    rng = np.random.default_rng(int(row["id"][1:]) + 1000)
    x = np.maximum(rng.standard_normal((n_images, d["Cin"], d["H"], d["W"])), 0).astype(np.float32)
    w = (rng.standard_normal((d["Cout"], d["Cin"], d["Kh"], d["Kw"])) * np.sqrt(2.0 / (d["Cin"] * d["Kh"] * d["Kw"]))).astype(np.float32)
    b = rng.standard_normal(d["Cout"]).astype(np.float32)
    if row["cls"].get("dtype", 0) == 1:
        x, w = _fp16_exact(x), _fp16_exact(w)
    return x, w, b


def _reference(x, w, b, pad, relu):
    y = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(), padding=pad)
    return (torch.relu(y) if relu else y).numpy()


def _err(y, ref):
    e = np.abs(y.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
    return float(e.max()), np.unravel_index(int(e.argmax()), e.shape)


@pytest.mark.parametrize("row", cc.CASES, ids=[r["id"] for r in cc.CASES])
def test_conv_class(hip, row):
    d, cls = row["desc"], cc.as_dict(cc.class_of_row(row))
    N, N2 = d["N"], row["N2"]
    relu = d.get("relu", True)
    plan = cc.make_plan(d, cls=hip.ConvPlan, device="cuda")
    got = tuple(plan.plan_class().values())
    assert got == cc.class_of_row(row), f"{row['id']} on this device: {cc.diff(got, cc.class_of_row(row))}"
    # one reference for both forwards: images are independent, the second forward runs them in another order
    n_ref = max(N, N2)
    x, w, b = _inputs(row, n_ref)
    ref = _reference(x, w, b, tuple(d["pad"]), relu)
    xd, wd, bd = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()
    plan.pack(wd)
    _, Cout, Ho, Wo = plan.out_shape()
    slots = None
    if cls["publishes_amax"]:
        slots = torch.zeros(hip.AMAX_SLOTS, dtype=torch.int32, device="cuda")
        plan.set_amax_io(None, slots)
    assert plan.can_pool == bool(cls["can_pool"]) and plan.can_pool_only == bool(cls["can_pool_only"]) and plan.publishes_amax == bool(cls["publishes_amax"])
    yp = torch.full((N, Cout, (Ho + 1) // 2, (Wo + 1) // 2), float("nan"), device="cuda") if cls["can_pool"] else None
    y = torch.full((N, Cout, Ho, Wo), float("nan"), device="cuda")
    plan.forward(xd[:N].contiguous(), bd, out=y, pool_out=yp)
    e, at = _err(y.cpu().numpy(), ref[:N])
    print(f"{row['id']} {plan.kernel}: max rel err {e:.3e} at {at}")
    assert e <= TOL, f"{row['id']} {plan.kernel}: max rel err {e:.3e} at {at}"
    if cls["can_pool"]:
        want_pool = hip.pool2d(y, (2, 2), (0, 0), (2, 2))
        assert torch.equal(yp, want_pool), f"{row['id']}: fused pooling differs from pooling y"
        if cls["can_pool_only"]:
            only = torch.full_like(yp, float("nan"))
            wsb = plan.ws.numel() * 4 if plan.ws is not None else 0
            hip._check(hip.lib().mscnn_conv2d_fwd_pool_f32(plan._p, hip._dev(xd[:N].contiguous()), hip._dev(plan.w), hip._dev(plan.packed), hip._dev(bd),
                                                           None, hip._dev(only), hip._dev(plan.ws), wsb, hip._stream()))
            assert torch.equal(only, want_pool), f"{row['id']}: the pooled-only call differs from pooling y"
    if slots is not None:
        assert slots.max().item() == y.abs().max().view(torch.int32).item(), f"{row['id']}: published max |y| is not the tensor's"
    # the same plan at another N of the same class, images rotated by one: stale workspace / output contents would show
    plan.set_batch(N2)
    assert tuple(plan.plan_class().values()) == cc.class_of_row(row)
    idx = [(i + 1) % n_ref for i in range(N2)]
    y2 = torch.full((N2, Cout, Ho, Wo), float("nan"), device="cuda")
    plan.forward(xd[idx].contiguous(), bd, out=y2)
    e2, at2 = _err(y2.cpu().numpy(), ref[idx])
    print(f"{row['id']} second forward at N = {N2}: max rel err {e2:.3e}")
    assert e2 <= TOL, f"{row['id']} {plan.kernel} after set_batch({N2}): max rel err {e2:.3e} at {at2}"
    torch.cuda.synchronize()
