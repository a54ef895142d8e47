"""The buffer contract of the C ABI (include/mscnn_hip.h), op family by op family: no op writes outside the buffers it is handed,
none writes its inputs, none depends on what an output or a workspace held on entry, and none reads outside its inputs.

Every test runs with tests/guarded.py in front of mscnn_amd.hipapi: each tensor a wrapper allocates sits between two 64 KB guard
bands and starts as 0xFF bytes (NaN / -1 / 255); the inputs are uploaded between guards of NaN (arithmetic ops), +inf (compare / select
ops) or 255 (uint8 images with pixels <= 200).  Each case compares VALUES with the oracle or a float64 reference under the bar
tests/test_gpu_ops.py uses for that op -- an unwritten output element or a consumed guard value is a NaN or an inf there -- and
then checks every guard and every input payload.  Wrappers that keep buffers across calls run twice on different inputs with their
workspace scribbled (0x5A) in between.  The second half covers what torch's 512-byte aligned allocations never reach: bases 4 bytes
past a 16-byte boundary (fall-backs and refusals) and grid-stride loops that take more than one trip."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import guarded  # noqa: E402

NAN, INF = np.nan, np.inf


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X: torch.cuda.is_available() is False")
    from mscnn_amd import hipapi
    hipapi.lib()
    return hipapi


class Guarded:
    def __init__(self, arena):
        self.arena = arena

    def inp(self, a, guard=NAN):
        return self.arena.input(np.ascontiguousarray(a), guard)

    def out(self, shape, dtype=torch.float32, fill=None):
        return self.arena.alloc(shape, dtype, fill)

    def off(self, t, elems=1):
        return self.arena.offset_view(t, elems)

    def owns(self, *tensors):
        """Each tensor starts a guarded allocation (the shim was in front of the wrapper that made it) and is no input."""
        for t in tensors:
            assert not self.arena.record(t).is_input

    def done(self):
        torch.cuda.synchronize()
        self.arena.check()


@pytest.fixture
def g(hip, monkeypatch):
    """Every allocation hipapi makes during the test comes from a fresh arena; the test ends with one more check of all of it."""
    arena = guarded.Arena("cuda")
    monkeypatch.setattr(hip, "torch", guarded.GuardedTorch(torch, arena))
    gg = Guarded(arena)
    yield gg
    gg.done()


def close(a, b, tol=1e-4):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.size == 0:
        return
    err = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    assert err.max() <= tol, f"max rel err {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}"      # (a NaN fails it)


def same(a, b):
    a = np.asarray(a); b = np.asarray(b)
    assert a.shape == b.shape and np.array_equal(a, b)      # (NaN != NaN: poison fails it)


def finite(*refs):
    """The reference must hold no NaN / inf of its own, or poison and data could not be told apart."""
    for r in refs:
        assert np.isfinite(np.asarray(r, np.float64)).all()


def cpu(t):
    return t.cpu().numpy()


def stream(hip):
    return hip._stream()


# ================================================================================================ convolution
def _fp16_exact(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def run_conv(hip, g, orc, N, Cin, H, W, Cout, k=(3, 3), pad=(1, 1), stride=(1, 1), group=1, relu=True, kernel=None, pool=False,
             exact16=False, relu_x=False, seed=1701, **plan_kw):
    """One plan, two forwards: x, then -2 x with the plan's workspace scribbled in between.  The convolution is linear, so ONE oracle
    run (without bias) gives both references: act(r + b) and act(-2 r + b), the factor being exact in fp32.  Returns what a
    follow-up (set_batch) needs."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, Cin, H, W))
    x = (np.maximum(x, 0) * 2.0 if relu_x else x).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin // group, *k)) * np.sqrt(2.0 / (Cin // group * k[0] * k[1]))).astype(np.float32)
    if exact16:
        x, w = _fp16_exact(x), _fp16_exact(w)
    b = rng.standard_normal(Cout).astype(np.float32)
    r = orc.conv2d(x, w, None, pad, stride, group)
    finite(r)
    act = (lambda v: np.maximum(v, 0)) if relu else (lambda v: v)
    bb = b[None, :, None, None]
    plan = hip.ConvPlan(N, Cin, H, W, Cout, k[0], k[1], pad, stride, group, relu, **plan_kw)
    assert kernel(plan.kernel) if callable(kernel) else plan.kernel == kernel, plan.kernel
    plan.pack(g.inp(w))
    bd = g.inp(b)
    for scale in (1.0, -2.0):
        if scale != 1.0:
            for t in (plan.ws,):
                if t is not None:
                    guarded.scribble(t, 0x5A)
        xs = (x * np.float32(scale)).astype(np.float32)
        Ho, Wo = plan.out_shape()[2:]
        yp = g.out((N, Cout, (Ho + 1) // 2, (Wo + 1) // 2)) if pool else None
        y = plan.forward(g.inp(xs), bd, pool_out=yp)
        g.owns(y, *[t for t in (plan.packed, plan.ws) if t is not None])
        g.done()
        close(cpu(y), act(np.float32(scale) * r + bb))
        if pool:
            assert plan.can_pool
            same(cpu(yp), orc.pool2d(cpu(y), (2, 2), (0, 0), (2, 2), "MAX"))
    return plan, x, bd, act(r + bb)


def is_igemm(name):
    return name.startswith("igemm_") and "_roi" not in name


@pytest.mark.parametrize("case", [(1, 12, 11, 19, 40), (2, 8, 10, 20, 130), (1, 24, 36, 120, 256)])
def test_conv_igemm(hip, g, orc, case):
    """Ragged Cin / Cout rows of a 128-row tile, batch 2, and the conv5-shaped plane whose tiles are split stream-K and summed by the
    fix-up launch (slabs in the plan's workspace)."""
    plan, *_ = run_conv(hip, g, orc, *case, algo=hip.ALGO_DIRECT, kernel=is_igemm)
    if case[4] == 256:
        assert plan.ws is not None and plan.ws.numel() > 0


def test_conv_igemm_1x1(hip, g, orc):
    run_conv(hip, g, orc, 1, 64, 10, 20, 96, (1, 1), (0, 0), kernel=lambda n: n.startswith("igemm_") and "k1x1" in n)


@pytest.mark.parametrize("case", [(2, 8, 67, 132, 64), (1, 8, 13, 37, 64)])
def test_conv_igemm_fused_pool(hip, g, orc, case):
    """The pooling epilogue at odd Ho / Wo: clipped ceil-mode windows on the last row / column, pooled rows of ragged tiles."""
    run_conv(hip, g, orc, *case, algo=hip.ALGO_DIRECT, kernel=is_igemm, pool=True)


@pytest.mark.parametrize("case", [(13, 16, 7, 7, 256, 0), (9, 8, 7, 5, 130, 0), (6, 24, 8, 4, 64, 1)])
def test_conv_roi_mode_igemm(hip, g, orc, case):
    """ROI-mode tiles (several whole ROI maps per tile, a ragged last group), then the ROI count changed both ways on the same plan."""
    R, Cin, H, W, Cout, pad = case
    plan, x, bd, ref = run_conv(hip, g, orc, R, Cin, H, W, Cout, pad=(pad, pad), algo=hip.ALGO_DIRECT,
                                kernel=lambda n: n.startswith("igemm_") and "_roi" in n)
    plan.set_batch(R + 7)
    more = np.arange(R + 7) % R
    close(cpu(plan.forward(g.inp(x[more]), bd)), ref[more])
    g.done()
    plan.set_batch(R - 5)
    assert hip.lib().mscnn_conv2d_workspace_bytes(plan._p) <= (plan.ws.numel() * 4 if plan.ws is not None else 0)
    close(cpu(plan.forward(g.inp(x[:R - 5]), bd)), ref[:R - 5])


@pytest.mark.parametrize("case", [(2, 8, 5, 5, 16, 1, 1), (2, 6, 9, 7, 4, 0, 2)])
def test_conv_direct_f32(hip, g, orc, case):
    N, Cin, H, W, Cout, pad, group = case
    run_conv(hip, g, orc, N, Cin, H, W, Cout, pad=(pad, pad), stride=(2, 2), group=group, kernel="direct_f32")


def test_conv_cin3(hip, g, orc):
    """Cin = 3: the small map stays on the igemm kernel (three channels zero-padded to a chunk; the VALU kernel takes maps of
    >= 4096 pixels with W % 4 == 0), the 130 x 36 one runs conv3x3_c3_valu_f32."""
    run_conv(hip, g, orc, 1, 3, 20, 33, 16, kernel=is_igemm)
    run_conv(hip, g, orc, 1, 3, 130, 36, 16, kernel="conv3x3_c3_valu_f32")


@pytest.mark.parametrize("case,flags,name", [
    ((1, 32, 18, 60, 9, (5, 5)), 0, "head4x4"), ((1, 16, 12, 20, 7, (5, 3)), 0, "head4x4"), ((2, 20, 40, 70, 6, (5, 3)), 0, "head4x4"),
    ((1, 64, 36, 120, 9, (5, 5)), 1024, "head_kwfold_shiftadd_f32"), ((2, 64, 12, 20, 7, (5, 3)), 16, "head_gemm_shiftadd_f32")])
def test_conv_proposal_heads(hip, g, orc, case, flags, name):
    N, Cin, H, W, Cout, k = case
    run_conv(hip, g, orc, N, Cin, H, W, Cout, k, (k[0] // 2, k[1] // 2), relu=False, relu_x=True, tune_flags=flags,
             kernel=lambda n: n.startswith(name))


@pytest.mark.parametrize("m", [2, 3, 4])
@pytest.mark.parametrize("case", [(1, 40, 13, 21, 130, 1), (1, 16, 11, 290, 24, 1)])
def test_conv_winograd_planes(hip, g, orc, case, m):
    """Odd H and W (partial tiles at the bottom / right edge), Cout ragged against the GEMM's row tile, 97 tile columns."""
    N, Cin, H, W, Cout, pad = case
    algo = {2: hip.ALGO_WINO_F2, 3: hip.ALGO_WINO_F3, 4: hip.ALGO_WINO_F4}[m]
    run_conv(hip, g, orc, N, Cin, H, W, Cout, pad=(pad, pad), algo=algo, kernel=f"winograd_f{m}x{m}_3x3", seed=4242)


@pytest.mark.parametrize("case,m", [((1, 40, 13, 21, 130), 2), ((1, 40, 12, 24, 130), 3), ((1, 24, 13, 21, 32), 4)])
def test_conv_winograd_fused_pool(hip, g, orc, case, m):
    algo = {2: hip.ALGO_WINO_F2, 3: hip.ALGO_WINO_F3, 4: hip.ALGO_WINO_F4}[m]
    run_conv(hip, g, orc, *case, algo=algo, kernel=f"winograd_f{m}x{m}_3x3", pool=True, seed=77)


@pytest.mark.parametrize("case", [(33, 32, 7, 5, 130, 0), (16, 32, 8, 4, 32, 1), (9, 64, 7, 7, 96, 0)])
def test_conv_winograd_f3_roi_maps(hip, g, orc, case):
    """F(3x3,3x3) on ROI maps: the igemm plane GEMM (Cout % 32 != 0), the wgemm one, and the 7x7 -> 5x5 plan with ragged planes
    (81 of 100 plane products per ROI); then a changed ROI count."""
    R, Cin, H, W, Cout, pad = case
    plan, x, bd, ref = run_conv(hip, g, orc, R, Cin, H, W, Cout, pad=(pad, pad), algo=hip.ALGO_WINO_F3, relu_x=True,
                                kernel="winograd_f3x3_3x3", seed=99)
    if (H, W, pad) == (7, 7, 0):
        assert sum(plan.plane_columns()) == 81 * R
    plan.set_batch(R + 7)
    more = np.arange(R + 7) % R
    close(cpu(plan.forward(g.inp(x[more]), bd)), ref[more])


@pytest.mark.parametrize("case", [(1, 32, 13, 21, 130, 1), (2, 64, 10, 14, 32, 1)])
def test_conv_winograd_x3(hip, g, orc, case):
    N, Cin, H, W, Cout, pad = case
    plan, *_ = run_conv(hip, g, orc, N, Cin, H, W, Cout, pad=(pad, pad), algo=hip.ALGO_WINO_F3_X3, tune_flags=4, seed=777,
                        kernel="winograd_f3x3_3x3_x3f16_128")
    assert plan.dtype == "f16x3"


def test_conv_direct_x3_fused_pool(hip, g, orc):
    plan, *_ = run_conv(hip, g, orc, 2, 32, 70, 130, 130, algo=hip.ALGO_WINO_F3_X3, relu_x=True, pool=True, seed=31,
                        kernel="igemm16x3_64x256_k3x3_tw32")
    assert plan.dtype == "f16x3"


@pytest.mark.parametrize("case,variant", [((1, 32, 12, 40, 130, 1, False), 0), ((1, 32, 12, 40, 130, 1, False), 202), ((1, 32, 12, 40, 130, 1, False), 203),
                                          ((1, 24, 13, 21, 64, 1, False), 0), ((2, 48, 18, 36, 96, 1, True), 0)])
def test_conv_f16_igemm(hip, g, orc, case, variant):
    """fp16 operands: with fp16-exact data the kernel computes the oracle's products, so the fp32 bar applies (tests/test_gpu_ops.py)."""
    N, Cin, H, W, Cout, pad, pooled = case
    plan, *_ = run_conv(hip, g, orc, N, Cin, H, W, Cout, pad=(pad, pad), algo=hip.ALGO_F16, tune_variant=variant, exact16=True, pool=pooled,
                        seed=31, kernel=lambda n: n.startswith("igemm16_") and n.endswith("_occ3") == (variant == 202)
                        and ("128x256" in n) == (variant == 203))
    assert plan.dtype == "f16"


@pytest.mark.parametrize("shape,variant,name", [((1, 8, 8, 32), 403, "winograd2x2_fused_k3x3_c64"), ((3, 40, 24, 64), 403, "winograd2x2_fused_k3x3_c64"),
                                                ((1, 8, 8, 128), 402, "wconv_64x512_k3x3"), ((3, 40, 16, 128), 402, "wconv_64x512_k3x3")])
def test_conv_one_launch_kernels(hip, g, orc, shape, variant, name):
    """conv1_2's shape class: the one-launch Winograd F(2x2,3x3) kernel and the ring kernel, with their fused pooling."""
    N, Cin, H, W = shape
    run_conv(hip, g, orc, N, Cin, H, W, 64, relu_x=True, pool=True, seed=29, tune_variant=variant, kernel=name,
             **({"algo": hip.ALGO_DIRECT} if variant == 402 else {}))


def test_conv_chain_f4(hip, g, orc):
    """Three chained F(4x4,3x3) layers: every plan's workspace is guarded, the activation between layers is written on request
    only, and a second frame runs through the same workspaces after they were scribbled."""
    N, C0, C1, C2, H, W = 2, 8, 16, 24, 40, 200
    rng = np.random.default_rng(5)
    chans = [C0, C1, C2, C1]
    plans, wn, bn = [], [], []
    for i in range(3):
        p = hip.ConvPlan(N, chans[i], H, W, chans[i + 1], 3, 3, (1, 1), relu=True, algo=hip.ALGO_WINO_F4)
        assert p.kernel == "winograd_f4x4_3x3"
        w = (rng.standard_normal((chans[i + 1], chans[i], 3, 3)) * np.sqrt(2.0 / (9 * chans[i]))).astype(np.float32)
        p.pack(g.inp(w))
        plans.append(p); wn.append(w); bn.append(rng.standard_normal(chans[i + 1]).astype(np.float32))
    a, b, c = plans
    assert a.can_chain(b) and b.can_chain(c) and c.can_pool_only
    bd = [g.inp(v) for v in bn]
    for frame in range(2):
        x = rng.standard_normal((N, C0, H, W)).astype(np.float32)
        r1 = orc.relu(orc.conv2d(x, wn[0], bn[0], (1, 1)))
        r2 = orc.relu(orc.conv2d(r1, wn[1], bn[1], (1, 1)))
        r3 = orc.relu(orc.conv2d(r2, wn[2], bn[2], (1, 1)))
        finite(r1, r2, r3)
        if frame:
            for p in plans:
                guarded.scribble(p.ws, 0x5A)
        a.forward_chain(g.inp(x), b, bd[0], write_y=False)
        y2 = b.forward_chain(None, c, bd[1], write_y=True)
        pool = g.out((N, chans[3], H // 2, W // 2))
        y3 = c.forward_chain(None, None, bd[2], pool_out=pool)
        g.done()
        close(cpu(y2), r2)
        close(cpu(y3), r3)
        same(cpu(pool), orc.pool2d(cpu(y3)))
        # the tail with only the pooled blob written
        a.forward_chain(g.inp(x), b, bd[0], write_y=False)
        b.forward_chain(None, c, bd[1], write_y=False)
        pool2 = g.out(tuple(pool.shape))
        assert c.forward_chain(None, None, bd[2], pool_out=pool2, write_y=False) is None
        g.done()
        assert torch.equal(pool2, pool)


def _kitti_like_rois(rng, R, H8, W8, batch=1):
    w = np.exp(rng.uniform(np.log(6), np.log(8 * W8 * 0.9), R)); h = w * rng.uniform(0.3, 1.6, R)
    x1 = rng.uniform(-40, 8 * W8 - 10, R); y1 = rng.uniform(-30, 8 * H8 - 10, R)
    rois = np.stack([rng.integers(0, batch, R).astype(np.float64), x1, y1, x1 + w, y1 + h], 1).astype(np.float32)
    rois[3, 3] = rois[3, 1] - 5.0
    rois[5, 1:] = [8 * W8 + 50, 10, 8 * W8 + 90, 60]
    rois[7, 1:] = [-300, -200, 8 * W8 + 300, 8 * H8 + 200]
    return rois


@pytest.mark.parametrize("case", [(37, 64, 24, 40, 96, 1), (21, 64, 20, 28, 64, 2)])
def test_conv_roipool_pair_fused(hip, g, orc, case):
    """Both ROI poolings fused into roi_c1's F(3x3,3x3) input stage: with the maps built inside the call (workspace sized by
    mscnn_conv2d_roipool_workspace_bytes) and with prepared maps (sized by mscnn_roipool_maps_bytes); the feature blob's guards
    are +inf -- a pooling window that strays past it wins every max."""
    R, Cc, H8, W8, Cout, batch = case
    rng = np.random.default_rng(R)
    feat = np.maximum(rng.standard_normal((batch, Cc, H8, W8)), 0).astype(np.float32) * 3.0
    rois = _kitti_like_rois(rng, R, H8, W8, batch)
    w = (rng.standard_normal((Cout, 2 * Cc, 3, 3)) * np.sqrt(2.0 / (2 * Cc * 9))).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32)
    pooled = np.concatenate([orc.roipool(feat, rois, 7, 7, 0.125, 0.0), orc.roipool(feat, rois, 7, 7, 0.125, 0.25)], 1)
    ref = orc.relu(orc.conv2d(pooled, w, b, (0, 0)))
    finite(pooled, ref)
    plan = hip.ConvPlan(R, 2 * Cc, 7, 7, Cout, 3, 3, (0, 0), relu=True, algo=hip.ALGO_WINO_F3)
    assert plan.kernel == "winograd_f3x3_3x3" and plan.can_fuse_roipool(Cc, 7, 7)
    plan.pack(g.inp(w))
    fd, rd, bd = g.inp(feat, INF), g.inp(rois), g.inp(b)
    close(cpu(plan.forward_roipool_pair(fd, rd, 0.125, 0.0, 0.25, bd)), ref)
    g.done()
    maps = hip.roipool_maps(fd)
    assert maps.numel() * 4 == hip.lib().mscnn_roipool_maps_bytes(batch, Cc, H8, W8)
    g.done()
    levels = [feat.transpose(0, 2, 3, 1)]                        # channel-last copy, then sliding maxima over 2 x 2, 4 x 4, 8 x 8 (clamped)
    for half in (1, 2, 4):
        p = levels[-1]
        yi, xi = np.minimum(np.arange(H8) + half, H8 - 1), np.minimum(np.arange(W8) + half, W8 - 1)
        levels.append(np.maximum(np.maximum(p, p[:, :, xi]), np.maximum(p[:, yi], p[:, yi][:, :, xi])))
    same(cpu(maps), np.concatenate([lv.reshape(-1) for lv in levels]))      # every word of the maps is written, none from outside feat
    guarded.scribble(plan.ws, 0x5A)
    close(cpu(plan.forward_roipool_pair(fd, rd, 0.125, 0.0, 0.25, bd, maps=maps)), ref)
    g.done()
    # the unfused pair into a guarded blob, bit-exact
    same(cpu(hip.roipool_pair(fd, rd, 7, 7, 0.125, 0.0, 0.25)), pooled)


# ================================================================================================ inner product
@pytest.mark.parametrize("M,N,K", [(5, 70, 33), (130, 192, 1000), (676, 2, 4096)])
def test_inner_product_f32(hip, g, orc, M, N, K):
    """The generic kernel (K % 4 != 0), the stream-K MFMA GEMM with ragged M and N, the small-N row kernel with a ragged last
    workgroup."""
    rng = np.random.default_rng(6)
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    ref = orc.inner_product(x, w, b)
    finite(ref)
    xd, wd, bd = g.inp(x), g.inp(w), g.inp(b)
    close(cpu(hip.inner_product(xd, wd, bd)), ref)
    close(cpu(hip.inner_product(xd, wd, None, relu=True)), orc.relu(orc.inner_product(x, w, None)))


def _ip_data(M, N, K, seed, exact16=False):
    rng = np.random.default_rng(seed)
    x = (np.maximum(rng.standard_normal((M, K)), 0) * 2.0).astype(np.float32)
    w = (rng.standard_normal((N, K)) * np.sqrt(2.0 / K)).astype(np.float32)
    if exact16:
        x, w = _fp16_exact(x), _fp16_exact(w)
    b = rng.standard_normal(N).astype(np.float32)
    ref = x.astype(np.float64) @ w.astype(np.float64).T + b
    finite(ref)
    return x, w, b, ref


def test_inner_product_wg(hip, g):
    """The plane-GEMM kernel: x re-packed inside the workspace, the last row tile reaching past M (193 rows of a 256-row tile)."""
    M, N, K = 193, 256, 64
    x, w, b, ref = _ip_data(M, N, K, M + N + K)
    assert hip.inner_product_wg_supported(M, N, K)
    xd, wd, bd = g.inp(x), g.inp(w), g.inp(b)
    y, wt = hip.inner_product_wg(xd, wd, bd)
    g.done()
    close(cpu(y), ref)
    same(cpu(wt), w.T)
    yr, _ = hip.inner_product_wg(xd, wd, bd, relu=True, wt=wt)
    close(cpu(yr), np.maximum(ref, 0))


def test_inner_product_x3(hip, g):
    M, N, K = 33, 128, 96
    x, w, b, ref = _ip_data(M, N, K, M + N)
    close(cpu(hip.inner_product_x3(g.inp(x), g.inp(w), g.inp(b), relu=True)), np.maximum(ref, 0))


@pytest.mark.parametrize("M,N,K", [(33, 64, 72), (257, 320, 1000)])
def test_inner_product_f16(hip, g, M, N, K):
    x, w, b, ref = _ip_data(M, N, K, M + N, exact16=True)
    close(cpu(hip.inner_product_f16(g.inp(x), g.inp(w), g.inp(b), relu=True)), np.maximum(ref, 0))


# ================================================================================================ elementwise, pooling
POOL_ROWS = [
    ((1, 64, 32, 48), (2, 2), (0, 0), (2, 2), "MAX"), ((2, 3, 9, 15), (2, 2), (0, 0), (2, 2), "MAX"), ((1, 2, 3, 5), (2, 2), (0, 0), (1, 1), "MAX"),
    ((1, 1, 3, 3), (3, 3), (2, 2), (2, 2), "MAX"), ((1, 4, 8, 8), (2, 2), (0, 0), (1, 1), "AVE"), ((1, 2, 7, 7), (3, 3), (1, 1), (2, 2), "AVE"),
    ((1, 3, 9, 15), (2, 2), (0, 0), (2, 2), "MAX"),
]


@pytest.mark.parametrize("shape,k,p,s,m", POOL_ROWS)
def test_pool(hip, g, orc, shape, k, p, s, m):
    x = np.random.default_rng(2).standard_normal(shape).astype(np.float32)
    ref = orc.pool2d(x, k, p, s, m)
    finite(ref)
    y = cpu(hip.pool2d(g.inp(x, INF if m == "MAX" else NAN), k, p, s, m))
    if m == "MAX":
        same(y, ref)
    else:
        close(y, ref, 1e-6)


def test_relu(hip, g, orc):
    rng = np.random.default_rng(1)
    for n in (1, 7, 1024, 4099):
        x = rng.standard_normal(n).astype(np.float32)
        y = hip.relu(g.inp(x))
        g.owns(y)
        same(cpu(y), orc.relu(x))
    x = rng.standard_normal(64).astype(np.float32)
    close(cpu(hip.relu(g.inp(x), 0.1)), orc.relu(x, 0.1), 1e-6)
    t = g.out(64)
    t.copy_(torch.from_numpy(x))
    hip.relu(t, inplace=True)
    same(cpu(t), orc.relu(x))


def test_concat(hip, g, orc):
    rng = np.random.default_rng(3)
    a = rng.standard_normal((5, 3, 7, 7)).astype(np.float32); b = rng.standard_normal((5, 4, 7, 7)).astype(np.float32)
    same(cpu(hip.concat_channels([g.inp(a), g.inp(b)])), orc.concat_channels([a, b]))


@pytest.mark.parametrize("shape", [(6, 5), (2, 5, 3, 7)])
def test_softmax(hip, g, shape):
    """Axis 1, also with inner > 1 (a channel stride of 21 floats): float64 numpy reference, 1e-6."""
    x = (np.random.default_rng(3).standard_normal(shape) * 3).astype(np.float32)
    e = np.exp(x.astype(np.float64) - x.astype(np.float64).max(1, keepdims=True))
    ref = e / e.sum(1, keepdims=True)
    finite(ref)
    close(cpu(hip.softmax(g.inp(x))), ref, 1e-6)


def test_eltwise(hip, g, orc):
    rng = np.random.default_rng(18)
    xs = [rng.standard_normal((37, 5)).astype(np.float32) for _ in range(3)]
    for op, cf in (("SUM", [0.33333333] * 3), ("SUM", None), ("PROD", None), ("MAX", None)):
        ds = [g.inp(x, INF if op == "MAX" else NAN) for x in xs]
        same(cpu(hip.eltwise(ds, op, cf)), orc.eltwise(xs, op, cf))


def _deconv2d(hip, x, w, bias, y, Cout, pad, stride, group):
    L = hip.lib()
    L.mscnn_deconv2d_fwd_f32.argtypes = [C.c_void_p] * 4 + [C.c_int] * 12 + [C.c_void_p]
    N, Cin, H, W = x.shape
    hip._check(L.mscnn_deconv2d_fwd_f32(hip._dev(x), hip._dev(w), hip._dev(bias), hip._dev(y), N, Cin, H, W, Cout, w.shape[2], w.shape[3],
                                        pad[0], pad[1], stride[0], stride[1], group, stream(hip)))


def test_deconv(hip, g, orc):
    """The depthwise 4x4 / stride 2 / pad 1 quad kernel (odd W: a last workgroup with idle lanes), the per-output depthwise kernel, and
    the general entry point with two groups."""
    rng = np.random.default_rng(23)
    x = np.maximum(rng.standard_normal((2, 8, 9, 11)), 0).astype(np.float32)
    w = (orc.bilinear_filler((8, 1, 4, 4)) * rng.uniform(0.5, 1.5, (8, 1, 1, 1))).astype(np.float32)
    b = rng.standard_normal(8).astype(np.float32)
    ref = orc.deconv2d(x, w, b, (1, 1), (2, 2), group=8)
    finite(ref)
    close(cpu(hip.deconv_depthwise(g.inp(x), g.inp(w), g.inp(b), (1, 1), (2, 2))), ref, 1e-6)
    w3 = rng.standard_normal((8, 1, 3, 3)).astype(np.float32)
    ref3 = orc.deconv2d(x, w3, None, (1, 1), (1, 1), group=8)
    finite(ref3)
    close(cpu(hip.deconv_depthwise(g.inp(x), g.inp(w3), None, (1, 1), (1, 1))), ref3, 1e-6)
    xg = rng.standard_normal((2, 6, 5, 7)).astype(np.float32)
    wg = (rng.standard_normal((6, 2, 3, 3)) * 0.3).astype(np.float32)          # w[Cin][Cout / group][Kh][Kw], Cout = 4
    bg = rng.standard_normal(4).astype(np.float32)
    refg = orc.deconv2d(xg, wg, bg, (1, 1), (2, 2), group=2)
    finite(refg)
    y = g.out(refg.shape)
    _deconv2d(hip, g.inp(xg), g.inp(wg), g.inp(bg), y, 4, (1, 1), (2, 2), 2)
    close(cpu(y), refg)


def test_parity_metric_ops(hip, g):
    """sum_squares, max_rel_diff, its strided form and store_words write one scalar (1 .. 4 words) each: float64 numpy references."""
    rng = np.random.default_rng(11)
    ref = (rng.standard_normal((5, 19, 33)) * 7).astype(np.float32)
    a = (ref + rng.standard_normal(ref.shape).astype(np.float32) * 1e-3).astype(np.float32)
    ad, rd = g.inp(a), g.inp(ref)
    ss = float((ref.astype(np.float64) ** 2).sum())
    assert abs(float(cpu(hip.sum_squares(rd))[0]) - ss) <= 1e-9 * ss
    want = (np.abs(a.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))).max()
    assert abs(float(cpu(hip.max_rel_diff(ad, rd))[0]) - want) <= 1e-6 * want
    rms = np.sqrt((ref.astype(np.float64) ** 2).mean())
    got = hip.max_rel_diff_strided(ad, 19 * 33, rd, 19 * 33, 5, 19 * 33, hip.sum_squares(rd), ref.size)
    w2 = (np.abs(a.astype(np.float64) - ref) / np.maximum(max(1.0, rms), np.abs(ref))).max()
    assert abs(float(cpu(got)[0]) - w2) <= 1e-5 * w2
    buf = g.out(8, torch.int32)
    hip.store_words(buf[2:], [11, -3, 2 ** 31 - 1])
    assert cpu(buf).tolist() == [-1, -1, 11, -3, 2 ** 31 - 1, -1, -1, -1]


# ================================================================================================ ROI pooling / align
def _random_rois(rng, R, img_h, img_w, batch=1):
    x1 = rng.uniform(-40, img_w, R); y1 = rng.uniform(-40, img_h, R)
    w = rng.uniform(1, 500, R); h = rng.uniform(1, 400, R)
    return np.stack([rng.integers(0, batch, R), x1, y1, x1 + w, y1 + h], 1).astype(np.float32)


def _roi_set(rng, R, scale, H, W):
    rois = _random_rois(rng, R, H / scale, W / scale, batch=2)
    rois[0] = [0, -500, -500, -300, -300]                       # fully outside
    rois[1] = [1, 0, 0, W / scale - 1, H / scale - 1]           # the whole map
    rois[2] = [0, 20, 20, 20, 20]
    return rois


@pytest.mark.parametrize("ph,pw,scale,pad", [(7, 7, 0.125, 0.0), (7, 7, 0.125, 0.25), (7, 5, 0.25, 0.25), (8, 4, 0.125, 0.0)])
def test_roipool(hip, g, orc, ph, pw, scale, pad):
    rng = np.random.default_rng(7)
    feat = rng.standard_normal((2, 24, 36, 120)).astype(np.float32)
    rois = _roi_set(rng, 97, scale, 36, 120)
    ref = orc.roipool(feat, rois, ph, pw, scale, pad)
    finite(ref)
    same(cpu(hip.roipool(g.inp(feat, INF), g.inp(rois), ph, pw, scale, pad)), ref)


def test_roipool_wide_rois(hip, g, orc):
    rng = np.random.default_rng(9)
    feat = np.maximum(rng.standard_normal((1, 16, 20, 700)), 0).astype(np.float32)
    rois = _random_rois(rng, 40, 80, 2800)
    rois[:, 3] = rois[:, 1] + rng.uniform(200, 2790, 40)
    rois[0] = [0, 0, 0, 2799, 79]; rois[1] = [0, -300, 5, 2500, 60]
    ref = orc.roipool(feat, rois, 7, 7, 0.25, 0.25)
    finite(ref)
    same(cpu(hip.roipool(g.inp(feat, INF), g.inp(rois), 7, 7, 0.25, 0.25)), ref)


@pytest.mark.parametrize("ph,pw,scale,C_,R", [(7, 7, 0.125, 24, 97), (7, 5, 0.25, 40, 33)])
def test_roipool_pair(hip, g, orc, ph, pw, scale, C_, R):
    rng = np.random.default_rng(11)
    feat = rng.standard_normal((2, C_, 36, 150)).astype(np.float32)
    rois = _roi_set(rng, R, scale, 36, 150)
    fd, rd = g.inp(feat, INF), g.inp(rois)
    for pa, pb in ((0.0, 0.25), (0.25, 0.0)):
        y = cpu(hip.roipool_pair(fd, rd, ph, pw, scale, pa, pb))
        same(y[:, :C_], orc.roipool(feat, rois, ph, pw, scale, pa))
        same(y[:, C_:], orc.roipool(feat, rois, ph, pw, scale, pb))


def test_roipool_channel_window(hip, g, orc):
    """c_total / c_offset: one call fills channels [16, 32) of a 48-channel blob; the windows on both sides keep their 0xFF bytes."""
    rng = np.random.default_rng(8)
    feat = rng.standard_normal((1, 16, 18, 60)).astype(np.float32)
    rois = _random_rois(rng, 10, 144, 480)
    out = g.out((10, 48, 7, 7))
    hip.roipool(g.inp(feat, INF), g.inp(rois), 7, 7, 0.125, 0.25, out=out, c_total=48, c_offset=16)
    g.done()
    same(cpu(out[:, 16:32]), orc.roipool(feat, rois, 7, 7, 0.125, 0.25))
    assert guarded.all_poison(out[:, :16].contiguous()) and guarded.all_poison(out[:, 32:].contiguous())


@pytest.mark.parametrize("ph,pw,scale,pad", [(7, 7, 0.125, 0.25), (4, 6, 0.25, 0.5)])
def test_roialign(hip, g, orc, ph, pw, scale, pad):
    rng = np.random.default_rng(17)
    feat = rng.standard_normal((2, 24, 36, 120)).astype(np.float32)
    rois = _random_rois(rng, 97, 36 / scale, 120 / scale, batch=2)
    rois[0] = [0, -500, -500, -300, -300]; rois[1, 3] = rois[1, 1] - 3
    ref = orc.roialign(feat, rois, ph, pw, scale, pad)
    finite(ref)
    same(cpu(hip.roialign(g.inp(feat), g.inp(rois), ph, pw, scale, pad)), ref)


# ================================================================================================ NMS, decode, final stages
def _clustered_boxes(rng, n):
    centers = rng.uniform(0, 1500, (max(1, n // 12), 2))
    c = centers[rng.integers(0, len(centers), n)] + rng.normal(0, 12, (n, 2))
    wh = rng.uniform(20, 200, (n, 2))
    return np.concatenate([c, wh], 1).astype(np.float32)


@pytest.mark.parametrize("n", [1, 64, 65, 500, 4033])
def test_nms_greedy(hip, g, orc, n):
    """keep and the bit-matrix workspace guarded; 4033 boxes take the tiled path (sort keys, kept list and state in the workspace)."""
    boxes = _clustered_boxes(np.random.default_rng(n), n)
    k = cpu(hip.nms_greedy(g.inp(boxes), 0.65, "IOU"))
    same(k, orc.nms_greedy(boxes, 0.65, "IOU"))
    assert n < 64 or (k.any() and not k.all())


@pytest.mark.parametrize("R", [1, 37, 4033])
def test_decode_bbox(hip, g, orc, R):
    rng = np.random.default_rng(12)
    prior = _random_rois(rng, R, 576, 1920)
    bbox = rng.standard_normal((R, 8)).astype(np.float32)
    ref = orc.decode_bbox(bbox, prior, (0, 0, 0, 0), (0.1, 0.1, 0.2, 0.2))
    finite(ref)
    same(cpu(hip.decode_bbox(g.inp(bbox), g.inp(prior), (0, 0, 0, 0), (0.1, 0.1, 0.2, 0.2))), ref)


def _final_inputs(R, seed):
    rng = np.random.default_rng(seed)
    b = _clustered_boxes(rng, R)
    props = np.concatenate([np.zeros((R, 1), np.float32), b[:, :2], b[:, :2] + b[:, 2:], rng.normal(0, 4, (R, 1)).astype(np.float32)], 1)
    props[::17, 5] = -11.0
    props[5::29, 3] = props[5::29, 1]
    bbox_pred = rng.standard_normal((R, 20)).astype(np.float32)
    cls_pred = (rng.standard_normal((R, 5)) * 2).astype(np.float32)
    cls_pred[3::7] = cls_pred[2::7][: len(cls_pred[3::7])]
    return bbox_pred, cls_pred, props.astype(np.float32)


@pytest.mark.parametrize("R", [1, 37, 4033])
def test_detections(hip, g, orc, R):
    bbox_pred, cls_pred, props = _final_inputs(R, R)
    kw = dict(cls_id=2, ratios=(576 / 375, 1920 / 1242), org_hw=(375, 1242))
    dref, iref = orc.detections(bbox_pred, cls_pred, props, **kw)
    finite(dref)
    n0 = len(g.arena.records)
    dets, ids = hip.detections(g.inp(bbox_pred), g.inp(cls_pred), g.inp(props), **kw)
    assert len(g.arena.records) == n0 + 3 + 4          # three inputs; dets, ids, count and the workspace
    g.done()
    same(cpu(ids), iref)
    close(cpu(dets), dref)


def _cascade_inputs(R, seed):
    rng = np.random.default_rng(seed)
    b = _clustered_boxes(rng, R)
    boxes = np.concatenate([np.zeros((R, 1), np.float32), b[:, :2] - 30, b[:, :2] + b[:, 2:] + 25], 1).astype(np.float32)
    props = np.concatenate([np.zeros((R, 1), np.float32), b[:, :2], b[:, :2] + b[:, 2:]], 1).astype(np.float32)
    props[3::31, 3] = props[3::31, 1] - 1
    prob = rng.uniform(0, 1, (R, 3)).astype(np.float32)
    prob[3::7] = prob[2::7][: len(prob[3::7])]
    return boxes, prob, props


@pytest.mark.parametrize("R", [1, 37, 4033])
def test_detections_cascade(hip, g, orc, R):
    boxes, prob, props = _cascade_inputs(R, 100 + R)
    kw = dict(cls_id=2, det_thr=0.2, ratios=(576 / 375, 1920 / 1242), org_hw=(375, 1242))
    dref, iref = orc.detections_cascade(boxes, prob, props, **kw)
    finite(dref)
    dets, ids = hip.detections_cascade(g.inp(boxes), g.inp(prob), g.inp(props), **kw)
    g.done()
    same(cpu(ids), iref)
    if R <= 4032:
        same(cpu(dets), dref)              # no transcendental in this stage: bit-exact
    else:
        close(cpu(dets), dref)


def _image_kw(i, overlap_odd=0.6):
    org = (375 + 40 * i, 1242 - 60 * i)
    return dict(ratios=(576 / org[0], 1920 / org[1]), org_hw=org, nms_overlap=0.5 if i % 2 == 0 else overlap_odd)


def test_detections_multi(hip, g, orc):
    """Two images (63 and 40 rows), two classes: every segment against the oracle on its row range; the pack and the workspace guarded."""
    rows, classes = [63, 40], [2, 3]
    parts = []
    for i, n in enumerate(rows):
        bp, cp, pr = _final_inputs(n, 11 + i)
        pr[:, 0] = i
        parts.append((bp[:, :16], cp[:, :4], pr))
    bbox_pred, cls_pred, props = (np.ascontiguousarray(np.concatenate([p[j] for p in parts], 0)) for j in range(3))
    segs = [dict(cls_id=c, **_image_kw(i)) for i in range(2) for c in classes]
    want = []
    for s, kw in enumerate(segs):
        i = s // 2
        sl = slice(sum(rows[:i]), sum(rows[:i + 1]))
        want.append(orc.detections(bbox_pred[sl], cls_pred[sl], props[sl], **kw))
        finite(want[-1][0])
    assert any(len(d) for d, _ in want)
    out = hip.detections_multi(g.inp(bbox_pred), g.inp(cls_pred), g.inp(props), 2, segs, max_rows_per_image=max(rows))
    g.done()
    for s, (dets, ids, row0, n) in enumerate(out):
        assert (row0, n) == (sum(rows[:s // 2]), rows[s // 2])
        same(ids, want[s][1])
        close(dets, want[s][0])


def test_detections_cascade_multi(hip, g, orc):
    rows, classes = [40, 64], [2, 3]
    parts = []
    for i, n in enumerate(rows):
        bx, pb, pr = _cascade_inputs(n, 200 + i)
        bx[:, 0] = i; pr[:, 0] = i
        parts.append((bx, pb, pr))
    boxes, prob, props = (np.ascontiguousarray(np.concatenate([p[j] for p in parts], 0)) for j in range(3))
    segs = [dict(cls_id=c, **_image_kw(i, 0.4)) for i in range(2) for c in classes]
    want = []
    for s, kw in enumerate(segs):
        i = s // 2
        sl = slice(sum(rows[:i]), sum(rows[:i + 1]))
        want.append(orc.detections_cascade(boxes[sl], prob[sl], props[sl], det_thr=0.25, **kw))
        finite(want[-1][0])
    assert any(len(d) for d, _ in want)
    out = hip.detections_cascade_multi([(g.inp(boxes), g.inp(prob), g.inp(props))], 2, segs, det_thr=0.25, max_rows_per_image=max(rows))
    g.done()
    for s, (dets, ids, row0, n) in enumerate(out):
        assert (row0, n) == (sum(rows[:s // 2]), rows[s // 2])
        same(ids, want[s][1])
        same(dets, want[s][0])


def test_proposals_multi(hip, g):
    """Against the numpy witness of the script (tests/proposals_witness.py), bit for bit; pack rows past a slot's count keep their
    zero fill, the pack's guards stay intact."""
    from proposals_witness import RATIOS, batch_witness, synth_props
    props = synth_props([65, 0, 130], 11)
    images = [dict(ratios=RATIOS[i % len(RATIOS)]) for i in range(3)]
    want = batch_witness(props, images)
    out, raw = hip.proposals_multi(g.inp(props), images, raw_pack=True)
    g.done()
    table = 16 * (len(images) + 1)
    dets = raw[table:table + 40 * len(props)].view(np.float64).reshape(-1, 5)
    ids = raw[table + 40 * len(props):table + 44 * len(props)].view(np.int32)
    for p, _, row0, n in out:                                   # rows of a slot past its count keep the zero fill they came with
        assert n == 0 or len(p) < n
        assert not dets[row0 + len(p):row0 + n].any() and not ids[row0 + len(p):row0 + n].any()
    for (p, rows, row0, n), (wp, wk, wrow0, wn) in zip(out, want):
        assert (row0, n) == (wrow0, wn)
        finite(wp)
        assert p.shape == wp.shape and np.array_equal(p.view(np.uint64), np.ascontiguousarray(wp, np.float64).view(np.uint64))
        same(rows, wk)


# ================================================================================================ pre-processing
def _rgb(h, w, seed):
    return np.random.default_rng(seed).integers(0, 201, (h, w, 3), dtype=np.uint8)      # pixels <= 200: the guards hold 255


def test_preprocess(hip, g, orc):
    img = _rgb(96, 130, 21)
    ref = orc.preprocess(img, 40, 57)
    finite(ref)
    same(cpu(hip.preprocess(g.inp(img, 255), 40, 57)), ref)


def test_preprocess_batch(hip, g, orc):
    orgs = [(96, 130), (50, 41), (33, 200)]
    frames = [_rgb(h, w, 30 + i) for i, (h, w) in enumerate(orgs)]
    ref = np.concatenate([orc.preprocess(f, 40, 57) for f in frames], 0)
    finite(ref)
    same(cpu(hip.preprocess_batch([g.inp(f, 255) for f in frames], 40, 57)), ref)


# ================================================================================================ BoxOutput through the wrapper
KITTI_HEADS = dict(shapes=[(18, 60), (18, 60), (9, 30), (9, 30), (5, 15), (5, 15), (3, 8)],
                   field=[60, 84, 120, 168, 240, 336, 480], ds=[8, 8, 16, 16, 32, 32, 64])


def _heads(rng, shapes, num=1, cls=5, bg_bias=0.0, sigma=2.0):
    out = []
    for (h, w) in shapes:
        t = rng.standard_normal((num, cls + 4, h, w)).astype(np.float32)
        t[:, :cls] *= sigma
        t[:, 0] += bg_bias
        t[:, cls:] *= 0.5
        out.append(t)
    return out


@pytest.mark.parametrize("one_pass,num", [(False, 1), (True, 2)])
def test_boxoutput_wrapper(hip, g, orc, one_pass, num):
    """hipapi.BoxOutput (per image, and one pass over a batch of two) on dense heads: its workspace, rois, props, anchor ids and count
    all come from the arena; the second frame runs after the workspace AND the outputs were scribbled."""
    kw = dict(fg_thr=-5.0, iou_thr=0.65, max_nms_num=2000, min_size=15.0)
    d = hip.make_boxoutput_desc(KITTI_HEADS["shapes"], num, 9, KITTI_HEADS["field"], KITTI_HEADS["field"], KITTI_HEADS["ds"], **kw)
    layer = hip.BoxOutput(d, one_pass=one_pass)
    for frame in range(2):
        heads = _heads(np.random.default_rng(1701 + frame), KITTI_HEADS["shapes"], num=num, bg_bias=-8.0)
        rois_r, props_r, _, nreal_r, aids_r = orc.boxoutput(heads, KITTI_HEADS["field"], KITTI_HEADS["field"], KITTI_HEADS["ds"],
                                                            with_anchor_ids=True, **kw)
        finite(rois_r, props_r)
        assert nreal_r > 100
        if frame:
            for t in (layer.ws, layer.rois, layer.props, layer.aids, layer.count):
                guarded.scribble(t, 0x5A)
        rois, props, aids, nreal = layer.forward([g.inp(h) for h in heads])
        g.owns(layer.ws, layer.rois, layer.props, layer.aids, layer.count)
        g.done()
        assert nreal == nreal_r
        same(cpu(aids), aids_r)
        same(cpu(rois), rois_r)
        same(cpu(props), props_r)


# ================================================================================================ alignment: fall-backs
# A base 4 bytes past a 16-byte boundary (arena.offset_view(t, 1)).  Ops that branch on alignment must give the aligned run's result
# on their scalar path; ops that refuse must do so before anything is stored through the pointer.
def _relu_raw(hip, x, y, slope=0.0):
    hip._check(hip.lib().mscnn_relu_fwd_f32(hip._dev(x), hip._dev(y), x.numel(), slope, stream(hip)))


@pytest.mark.parametrize("which", ["x", "y", "both"])
def test_align_relu(hip, g, orc, which):
    x = np.random.default_rng(1).standard_normal(1028).astype(np.float32)      # count % 4 == 0: the aligned run is the float4 kernel
    xd, y = g.inp(x), g.out(1028)
    if which in ("x", "both"):
        xd = g.off(xd)
    if which in ("y", "both"):
        y = g.off(y)
    _relu_raw(hip, xd, y)
    same(cpu(y), orc.relu(x))


@pytest.mark.parametrize("which", ["x", "y"])
def test_align_pool_fast_path(hip, g, orc, which):
    shape = (1, 4, 8, 16)
    x = np.random.default_rng(2).standard_normal(shape).astype(np.float32)
    xd, y = g.inp(x, INF), g.out((1, 4, 4, 8))
    if which == "x":
        xd = g.off(xd)
    else:
        y = g.off(y)
    hip._check(hip.lib().mscnn_pool2d_fwd_f32(hip._dev(xd), hip._dev(y), 1, 4, 8, 16, 2, 2, 0, 0, 2, 2, 0, stream(hip)))
    g.done()
    same(cpu(y), orc.pool2d(x))
    same(cpu(y), cpu(hip.pool2d(g.inp(x, INF))))                  # the aligned run (the float4 fast path)


@pytest.mark.parametrize("which", ["x", "w"])
def test_align_inner_product(hip, g, orc, which):
    """(7, 128, 256): aligned it runs the MFMA GEMM, with x or w 4 bytes off the generic kernel."""
    M, N, K = 7, 128, 256
    rng = np.random.default_rng(6)
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    ref = orc.inner_product(x, w, b)
    finite(ref)
    xd, wd, bd = g.inp(x), g.inp(w), g.inp(b)
    y0 = cpu(hip.inner_product(xd, wd, bd))
    y1 = cpu(hip.inner_product(g.off(xd) if which == "x" else xd, g.off(wd) if which == "w" else wd, bd))
    close(y0, ref)
    close(y1, ref)
    close(y1, y0)


@pytest.mark.parametrize("which", ["x", "y"])
def test_align_wino_f3_roi_transforms(hip, g, orc, which):
    """The small-map F(3x3,3x3) transforms stage whole ROI runs with float4 copies where the base allows it and with scalars where
    it does not: the same bits either way."""
    R, Cin, H, W, Cout, pad = 16, 32, 8, 4, 32, 1
    rng = np.random.default_rng(99)
    x = (np.maximum(rng.standard_normal((R, Cin, H, W)), 0) * 2.0).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, 3, 3)) * np.sqrt(2.0 / (Cin * 9))).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32)
    ref = orc.relu(orc.conv2d(x, w, b, (pad, pad)))
    finite(ref)
    plan = hip.ConvPlan(R, Cin, H, W, Cout, 3, 3, (pad, pad), relu=True, algo=hip.ALGO_WINO_F3)
    assert plan.kernel == "winograd_f3x3_3x3"
    plan.pack(g.inp(w))
    xd, bd = g.inp(x), g.inp(b)
    y0 = plan.forward(xd, bd).clone()
    y = g.off(g.out(tuple(y0.shape))) if which == "y" else None
    y1 = plan.forward(g.off(xd) if which == "x" else xd, bd, out=y)
    g.done()
    close(cpu(y0), ref)
    assert torch.equal(y1, y0)


@pytest.mark.parametrize("which", ["x", "y", "y_pool"])
def test_align_wino_f4_vector_transforms(hip, g, orc, which):
    """W % 4 == 0: aligned, the float4 transforms run; with x, y or the pooled map 4 bytes off the scalar kernels do."""
    N, Cin, H, W, Cout = 1, 32, 24, 64, 48
    rng = np.random.default_rng(3)
    x = rng.standard_normal((N, Cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, 3, 3)) * np.sqrt(2.0 / (Cin * 9))).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32)
    ref = orc.relu(orc.conv2d(x, w, b, (1, 1)))
    finite(ref)
    plan = hip.ConvPlan(N, Cin, H, W, Cout, 3, 3, (1, 1), relu=True, algo=hip.ALGO_WINO_F4)
    assert plan.kernel == "winograd_f4x4_3x3"
    plan.pack(g.inp(w))
    xd, bd = g.inp(x), g.inp(b)
    p0 = g.out((N, Cout, H // 2, W // 2))
    y0 = plan.forward(xd, bd, pool_out=p0).clone()
    y = g.off(g.out(tuple(y0.shape))) if which == "y" else None
    p1 = g.out(tuple(p0.shape))
    p1 = g.off(p1) if which == "y_pool" else p1
    y1 = plan.forward(g.off(xd) if which == "x" else xd, bd, out=y, pool_out=p1)
    g.done()
    close(cpu(y0), ref)
    close(cpu(y1), cpu(y0))
    close(cpu(y1), ref)
    same(cpu(p1), orc.pool2d(cpu(y1)))
    same(cpu(p0), orc.pool2d(cpu(y0)))


def test_align_deconv_up2(hip, g, orc):
    """The 4x4 / stride 2 quad kernel stores float2 pairs: a y that is only 4-byte aligned takes the per-output kernel."""
    rng = np.random.default_rng(23)
    x = np.maximum(rng.standard_normal((1, 4, 6, 10)), 0).astype(np.float32)
    w = orc.bilinear_filler((4, 1, 4, 4)).astype(np.float32)
    ref = orc.deconv2d(x, w, None, (1, 1), (2, 2), group=4)
    finite(ref)
    y = g.off(g.out(ref.shape))
    hip._check(hip.lib().mscnn_deconv_depthwise_fwd_f32(hip._dev(g.inp(x)), hip._dev(g.inp(w)), None, hip._dev(y), 1, 4, 6, 10, 4, 4, 1, 1, 2, 2,
                                                        stream(hip)))
    close(cpu(y), ref, 1e-6)


# ================================================================================================ alignment: refusals
def _refused(hip, g, call, *outputs):
    """`call` must raise before anything is stored: every output still holds its poison, every guard is intact."""
    with pytest.raises(hip.MscnnError, match="align"):
        call()
    g.done()
    for t in outputs:
        assert guarded.all_poison(t)


def test_refuse_conv_cin3(hip, g):
    rng = np.random.default_rng(1)
    plan = hip.ConvPlan(1, 3, 130, 36, 16, 3, 3, (1, 1), relu=True)
    assert plan.kernel == "conv3x3_c3_valu_f32"
    plan.pack(g.inp(rng.standard_normal((16, 3, 3, 3)).astype(np.float32)))
    x = g.inp(rng.standard_normal((1, 3, 130, 36)).astype(np.float32))
    y = g.out((1, 16, 130, 36))
    _refused(hip, g, lambda: plan.forward(g.off(x), None, out=y), y)
    yo = g.off(g.out((1, 16, 130, 36)))
    _refused(hip, g, lambda: plan.forward(x, None, out=yo), yo)


def test_refuse_wf2conv(hip, g):
    rng = np.random.default_rng(2)
    plan = hip.ConvPlan(1, 8, 8, 32, 64, 3, 3, (1, 1), relu=True, tune_variant=403)
    assert plan.kernel == "winograd2x2_fused_k3x3_c64"
    plan.pack(g.inp(rng.standard_normal((64, 8, 3, 3)).astype(np.float32)))
    x = g.inp(rng.standard_normal((1, 8, 8, 32)).astype(np.float32))
    y = g.out((1, 64, 8, 32))
    _refused(hip, g, lambda: plan.forward(g.off(x), None, out=y), y)
    yo = g.off(g.out((1, 64, 8, 32)))
    _refused(hip, g, lambda: plan.forward(x, None, out=yo), yo)


def test_refuse_inner_products(hip, g):
    """f16, x3 and wg InnerProduct need a 16-byte aligned x (float4 row loads)."""
    L = hip.lib()
    rng = np.random.default_rng(3)
    M, N, K = 33, 128, 96
    x = g.off(g.inp(rng.standard_normal((M, K)).astype(np.float32)))
    w = g.inp(rng.standard_normal((N, K)).astype(np.float32))
    y = g.out((M, N))
    w16 = g.out(N * K, torch.float16)
    hip._check(L.mscnn_inner_product_pack_f16(hip._dev(w), hip._dev(w16), N, K, stream(hip)))
    _refused(hip, g, lambda: hip._check(L.mscnn_inner_product_fwd_f16(hip._dev(x), hip._dev(w16), None, hip._dev(y), M, N, K, 0, stream(hip))), y)
    packed = g.out(L.mscnn_inner_product_x3_packed_bytes(N, K), torch.uint8)
    hip._check(L.mscnn_inner_product_x3_pack(hip._dev(w), hip._dev(packed), N, K, stream(hip)))
    wb = L.mscnn_inner_product_x3_workspace_bytes(M, N, K)
    ws = g.out(wb, torch.uint8)
    _refused(hip, g, lambda: hip._check(L.mscnn_inner_product_x3_fwd(hip._dev(x), hip._dev(packed), None, hip._dev(y), M, N, K, 0, None, hip._dev(ws), wb,
                                                                    stream(hip))), y, ws)
    M2, N2, K2 = 193, 256, 64
    x2 = g.off(g.inp(rng.standard_normal((M2, K2)).astype(np.float32)))
    w2 = g.inp(rng.standard_normal((N2, K2)).astype(np.float32))
    y2 = g.out((M2, N2))
    _refused(hip, g, lambda: hip.inner_product_wg(x2, w2, None, out=y2), y2)


def test_refuse_nms_and_proposals(hip, g):
    L = hip.lib()
    boxes = g.off(g.inp(_clustered_boxes(np.random.default_rng(5), 65)))
    keep = g.out(65, torch.uint8)
    wb = L.mscnn_nms_workspace_bytes(65)
    ws = g.out(wb, torch.uint8)
    _refused(hip, g, lambda: hip._check(L.mscnn_nms_greedy_f32(hip._dev(boxes), 65, 0.65, 0, hip._dev(keep), hip._dev(ws), wb, stream(hip))), keep, ws)
    from proposals_witness import RATIOS, synth_props
    props = synth_props([20], 3)
    pack = g.out(L.mscnn_proposals_multi_pack_bytes(1, len(props)), torch.uint8)
    _refused(hip, g, lambda: hip.proposals_multi(g.off(g.inp(props)), [dict(ratios=RATIOS[0])], pack=pack), pack)
    pack2 = g.off(g.out(L.mscnn_proposals_multi_pack_bytes(1, len(props)) + 4, torch.uint8), 4)
    _refused(hip, g, lambda: hip.proposals_multi(g.inp(props), [dict(ratios=RATIOS[0])], pack=pack2), pack2)


def test_refuse_roipool_maps_and_planes(hip, g):
    """The fused ROI pooling: maps and transform planes (the start of the plan's workspace) must be 16-byte aligned."""
    L = hip.lib()
    rng = np.random.default_rng(7)
    R, Cc, H8, W8, Cout = 21, 64, 20, 28, 64
    feat = g.inp(np.maximum(rng.standard_normal((1, Cc, H8, W8)), 0).astype(np.float32), INF)
    maps = g.off(g.out(L.mscnn_roipool_maps_bytes(1, Cc, H8, W8) // 4))
    _refused(hip, g, lambda: hip._check(L.mscnn_roipool_maps_build_f32(hip._dev(feat), hip._dev(maps), 1, Cc, H8, W8, stream(hip))), maps)
    plan = hip.ConvPlan(R, 2 * Cc, 7, 7, Cout, 3, 3, (0, 0), relu=True, algo=hip.ALGO_WINO_F3)
    assert plan.can_fuse_roipool(Cc, 7, 7)
    plan.pack(g.inp((rng.standard_normal((Cout, 2 * Cc, 3, 3)) * 0.05).astype(np.float32)))
    good = hip.roipool_maps(feat)
    need = L.mscnn_conv2d_roipool_workspace_bytes(plan._p, 1, Cc, H8, W8)      # (what the wrapper asks for, or it would re-allocate)
    plan.ws = g.off(g.out((need + 3) // 4))
    y = g.out(plan.out_shape())
    rois = g.inp(_kitti_like_rois(rng, R, H8, W8))
    _refused(hip, g, lambda: plan.forward_roipool_pair(feat, rois, 0.125, 0.0, 0.25, None, out=y, maps=good), y, plan.ws)


def test_refuse_wino_outputs(hip, g):
    """The chained F(4x4,3x3) output stage stores float4 rows of y, the F(2x2,3x3) and the pooling F(3x3,3x3) output transforms
    float2 pairs: an y that does not allow them is refused, and nothing is stored through it."""
    rng = np.random.default_rng(9)
    N, C0, C1, H, W = 1, 8, 16, 16, 40
    a = hip.ConvPlan(N, C0, H, W, C1, 3, 3, (1, 1), relu=True, algo=hip.ALGO_WINO_F4)
    b = hip.ConvPlan(N, C1, H, W, C0, 3, 3, (1, 1), relu=True, algo=hip.ALGO_WINO_F4)
    assert a.can_chain(b)
    a.pack(g.inp((rng.standard_normal((C1, C0, 3, 3)) * 0.1).astype(np.float32)))
    x = g.inp(rng.standard_normal((N, C0, H, W)).astype(np.float32))
    y = g.off(g.out((N, C1, H, W)))
    _refused(hip, g, lambda: a.forward_chain(x, b, None, out=y), y)
    assert guarded.all_poison(a.ws) and guarded.all_poison(b.ws)      # refused before the input transform was launched
    for algo, shape in ((hip.ALGO_WINO_F2, (1, 16, 8, 12, 24)), (hip.ALGO_WINO_F3, (1, 40, 12, 24, 32))):
        n, cin, h, w_, cout = shape
        p = hip.ConvPlan(n, cin, h, w_, cout, 3, 3, (1, 1), relu=True, algo=algo)
        assert p.kernel.startswith("winograd_f") and p.can_pool
        p.pack(g.inp((rng.standard_normal((cout, cin, 3, 3)) * 0.1).astype(np.float32)))
        xx = g.inp(rng.standard_normal((n, cin, h, w_)).astype(np.float32))
        yo = g.off(g.out((n, cout, h, w_)))
        yp = g.out((n, cout, h // 2, w_ // 2))
        _refused(hip, g, lambda: p.forward(xx, None, out=yo, pool_out=yp), yo, yp, p.ws)      # (p.ws: not even the input transform ran)


def test_refuse_conv_split_fp16_x(hip, g):
    """The split-fp16 forms measure max |x| with 16-byte loads (and stage small maps with float4): a 4-byte aligned x is refused
    before that pass -- on whole planes, on ROI maps and with max |x| handed over (no pass at all)."""
    rng = np.random.default_rng(4)
    for shape, pad in (((2, 64, 10, 14, 32), 1), ((16, 32, 8, 4, 32), 1)):
        N, Cin, H, W, Cout = shape
        plan = hip.ConvPlan(N, Cin, H, W, Cout, 3, 3, (pad, pad), relu=True, algo=hip.ALGO_WINO_F3_X3, tune_flags=4)
        assert plan.kernel.startswith("winograd_f3x3_3x3_x3f16") and plan.dtype == "f16x3"
        plan.pack(g.inp((rng.standard_normal((Cout, Cin, 3, 3)) * 0.1).astype(np.float32)))
        x = g.off(g.inp(rng.standard_normal((N, Cin, H, W)).astype(np.float32)))
        for bound in (False, True):
            if bound:
                slots = g.out(hip.AMAX_SLOTS, torch.int32, fill=0)
                slots[3] = torch.tensor(8.0, dtype=torch.float32).view(torch.int32)
                plan.set_amax_io(slots, None)
            guarded.scribble(plan.ws, 0xFF)
            y = g.out(plan.out_shape())
            _refused(hip, g, lambda: plan.forward(x, None, out=y), y, plan.ws)
    w = g.off(g.inp(rng.standard_normal((32, 32, 3, 3)).astype(np.float32)))      # ... and the weights' own max pass at pack time
    packed = plan.packed
    guarded.scribble(packed, 0xFF)
    _refused(hip, g, lambda: plan.pack(w), packed)


def test_refuse_workspaces_and_packed_weights(hip, g):
    """Workspaces and packed weights are read and written with 16-byte accesses by every kernel family: a base that is not 16-byte
    aligned is refused before the first launch, whatever the family."""
    L = hip.lib()
    rng = np.random.default_rng(5)
    for kw in (dict(algo=hip.ALGO_DIRECT), dict(algo=hip.ALGO_WINO_F3), dict(algo=hip.ALGO_WINO_F4)):
        plan = hip.ConvPlan(1, 24, 36, 120, 256, 3, 3, (1, 1), relu=True, **kw)
        assert plan.ws is not None and plan.packed is not None, plan.kernel
        w = g.inp((rng.standard_normal((256, 24, 3, 3)) * 0.1).astype(np.float32))
        good = plan.packed
        plan.packed = g.off(g.out(good.numel()))
        _refused(hip, g, lambda: plan.pack(w), plan.packed)
        plan.packed = good
        plan.pack(w)
        x = g.inp(rng.standard_normal((1, 24, 36, 120)).astype(np.float32))
        plan.ws = g.off(g.out(plan.ws.numel()))
        y = g.out(plan.out_shape())
        _refused(hip, g, lambda: plan.forward(x, None, out=y), y, plan.ws)
    d = hip.make_boxoutput_desc(KITTI_HEADS["shapes"], 1, 9, KITTI_HEADS["field"], KITTI_HEADS["field"], KITTI_HEADS["ds"])
    for one_pass in (False, True):
        layer = hip.BoxOutput(d, one_pass=one_pass)
        layer.ws = g.off(g.out(layer.ws.numel() + 4, torch.uint8), 4)
        heads = [g.inp(h) for h in _heads(rng, KITTI_HEADS["shapes"], bg_bias=-8.0)]
        _refused(hip, g, lambda: layer.forward_async(heads), layer.rois, layer.props, layer.aids, layer.ws)
    boxes = g.inp(_clustered_boxes(rng, 65))
    keep = g.out(65, torch.uint8)
    wb = L.mscnn_nms_workspace_bytes(65)
    ws = g.off(g.out(wb + 4, torch.uint8), 4)
    _refused(hip, g, lambda: hip._check(L.mscnn_nms_greedy_f32(hip._dev(boxes), 65, 0.65, 0, hip._dev(keep), hip._dev(ws), wb, stream(hip))), keep, ws)
    M, N, K = 193, 256, 64
    xw = g.inp(rng.standard_normal((M, K)).astype(np.float32))
    wt = g.off(g.out((K, N)))
    y = g.out((M, N))
    ww = g.inp(rng.standard_normal((N, K)).astype(np.float32))
    _refused(hip, g, lambda: hip.inner_product_wg(xw, ww, None, wt=wt, out=y), y)


@pytest.mark.parametrize("case,k,name", [((1, 12, 11, 19, 40), (3, 3), "igemm_"), ((1, 16, 12, 20, 7), (5, 3), "head4x4")])
def test_align_four_byte_conv_kernels(hip, g, orc, case, k, name):
    """The direct implicit-GEMM and the M = 4 head kernels load x and store y one dword at a time: blobs that are only 4-byte
    aligned are theirs to take, with the aligned run's result."""
    N, Cin, H, W, Cout = case
    pad = (k[0] // 2, k[1] // 2)
    rng = np.random.default_rng(1701)
    x = rng.standard_normal((N, Cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, *k)) * np.sqrt(2.0 / (Cin * k[0] * k[1]))).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32)
    ref = orc.conv2d(x, w, b, pad)
    finite(ref)
    plan = hip.ConvPlan(N, Cin, H, W, Cout, k[0], k[1], pad, algo=hip.ALGO_DIRECT)
    assert plan.kernel.startswith(name) and "_vec" not in plan.kernel
    plan.pack(g.inp(w))
    xd, bd = g.inp(x), g.off(g.inp(b))
    y0 = plan.forward(xd, bd).clone()
    y1 = plan.forward(g.off(xd), bd, out=g.off(g.out(tuple(y0.shape))))
    g.done()
    close(cpu(y0), ref)
    assert torch.equal(y1, y0)


# ================================================================================================ grid-stride loops
# The bandwidth kernels of elementwise.hip run at most 2048 workgroups of 256 threads = 524,288 work items per trip.
GRID_ITEMS = 2048 * 256


@pytest.mark.parametrize("n", [2_400_004, 600_001])
def test_stride_relu(hip, g, orc, n):
    """2,400,004 floats = 600,001 float4 items of the vector kernel; 600,001 floats run the scalar kernel (count % 4 != 0)."""
    assert (n // 4 if n % 4 == 0 else n) > GRID_ITEMS
    x = np.random.default_rng(n).standard_normal(n).astype(np.float32)
    same(cpu(hip.relu(g.inp(x))), np.maximum(x, 0))


@pytest.mark.parametrize("shape,k,s", [((1, 8, 300, 260), (3, 3), (1, 1)), ((1, 32, 280, 560), (2, 2), (2, 2))])
def test_stride_pool(hip, g, orc, shape, k, s):
    """The general kernel (one output per item: 615,072) and the 2x2 fast path (two outputs per item: 627,200 items)."""
    x = np.random.default_rng(4).standard_normal(shape).astype(np.float32)
    ref = orc.pool2d(x, k, (0, 0), s, "MAX")
    assert ref.size // (2 if k == (2, 2) else 1) > GRID_ITEMS
    same(cpu(hip.pool2d(g.inp(x, INF), k, (0, 0), s, "MAX")), ref)


def test_stride_concat(hip, g):
    rng = np.random.default_rng(5)
    a = rng.standard_normal((2, 5, 300, 200)).astype(np.float32); b = rng.standard_normal((2, 1, 300, 200)).astype(np.float32)
    assert a.size > GRID_ITEMS
    same(cpu(hip.concat_channels([g.inp(a), g.inp(b)])), np.concatenate([a, b], 1))


def test_stride_softmax(hip, g):
    x = (np.random.default_rng(6).standard_normal((2, 3, 300, 1000)) * 3).astype(np.float32)
    assert x.size // 3 > GRID_ITEMS
    e = np.exp(x.astype(np.float64) - x.astype(np.float64).max(1, keepdims=True))
    close(cpu(hip.softmax(g.inp(x))), e / e.sum(1, keepdims=True), 1e-6)


def test_stride_eltwise(hip, g, orc):
    rng = np.random.default_rng(7)
    xs = [rng.standard_normal(600_001).astype(np.float32) for _ in range(2)]
    same(cpu(hip.eltwise([g.inp(x) for x in xs], "SUM", [0.5, -1.5])), orc.eltwise(xs, "SUM", [0.5, -1.5]))
    same(cpu(hip.eltwise([g.inp(x, INF) for x in xs], "MAX")), np.maximum(xs[0], xs[1]))


def test_stride_deconv(hip, g, orc):
    """The per-output depthwise kernel (3x3 / stride 1: 608,400 outputs) and the generic one (two groups, 640,000 outputs)."""
    rng = np.random.default_rng(8)
    x = rng.standard_normal((1, 4, 390, 390)).astype(np.float32)
    w = rng.standard_normal((4, 1, 3, 3)).astype(np.float32)
    ref = orc.deconv2d(x, w, None, (1, 1), (1, 1), group=4)
    assert ref.size > GRID_ITEMS
    finite(ref)
    close(cpu(hip.deconv_depthwise(g.inp(x), g.inp(w), None, (1, 1), (1, 1))), ref, 1e-6)
    xg = rng.standard_normal((1, 4, 200, 200)).astype(np.float32)
    wg = rng.standard_normal((4, 2, 2, 2)).astype(np.float32)
    refg = orc.deconv2d(xg, wg, None, (0, 0), (2, 2), group=2)
    assert refg.size > GRID_ITEMS
    finite(refg)
    y = g.out(refg.shape)
    _deconv2d(hip, g.inp(xg), g.inp(wg), None, y, 4, (0, 0), (2, 2), 2)
    close(cpu(y), refg)
