"""The gated cases of tests/test_gpu_stream_contract.py: one per op family, at the shapes tests/test_gpu_buffer_contract.py uses for
that family (its builders are imported from it, so the inputs are the same valid ones), each naming the C-ABI functions it runs.

Importing this module needs neither torch nor a GPU: tests/test_stream_cases_cpu.py reads CASES and NO_GATED_CASE to hold the table
against include/mscnn_hip.h.  Everything else happens inside the callables.

WRAPPERS THAT SYNCHRONISE.  These mscnn_amd.hipapi wrappers wait for the device themselves, so their cases call the C ABI
directly (as _deconv2d of the buffer-contract file does) and keep the `busy` assertion:
    inner_product_wg        torch.cuda.current_stream().synchronize() behind the forward (its workspace dies with the call)
    conv2d                  the same, behind plan.forward (the plan's buffers die with the plan)
    preprocess, preprocess_batch, preprocess_views      the same (their workspace dies with the frame)
    rois_ingest             torch.cuda.synchronize() in front of its four .cpu() reads
    BoxOutput.forward       self.count.tolist(); the case uses forward_async
    detections, detections_cascade      int(count.item())
    detections_multi, detections_cascade_multi, proposals_multi, Candidates.merge*      pack.cpu() in _read_multi_pack / _read_pack
    nms_greedy              none, but keep[:n].bool() is a torch kernel behind the op: harmless, it runs on the same stream
ConvPlan.__del__ (mscnn_conv2d_plan_destroy) frees host memory only and takes no stream."""
import ctypes as C
import functools

import numpy as np

from tests.streams import Case


def _bc():
    from tests import test_gpu_buffer_contract as bc
    return bc


def _torch():
    import torch
    return torch


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _empty(shape, dtype=None):
    torch = _torch()
    return torch.empty(shape, dtype=dtype or torch.float32, device="cuda")


def _zeros(shape, dtype=None):
    torch = _torch()
    return torch.zeros(shape, dtype=dtype or torch.float32, device="cuda")


def close(a, b, tol=1e-4):
    _bc().close(a, b, tol)


def same(a, b):
    _bc().same(a, b)


CASES = []


def case(*a, **kw):
    CASES.append(Case(*a, **kw))


# ================================================================================================ convolution
def _conv_case(name, shape, kernel, k=(3, 3), pad=(1, 1), stride=(1, 1), group=1, relu=True, pool=False, exact16=False, relu_x=False,
               plain=False, split=None, algo=None, **plan_kw):
    """One plan; run() packs the weights and runs one forward (mscnn_conv2d_pack_weights + mscnn_conv2d_fwd_pool_f32, or
    mscnn_conv2d_fwd_f32 with plain).  The packed weights and the workspace are scribbled behind the call.  split: None, or what
    the plan's wg_split class field must be (0: whole tiles, non-zero: tiles split between workgroups)."""
    N, Cin, H, W, Cout = shape

    def draw(seed):
        rng = np.random.default_rng(seed)
        x = rng.standard_normal((N, Cin, H, W))
        x = (np.maximum(x, 0) * 2.0 if relu_x else x).astype(np.float32)
        w = (rng.standard_normal((Cout, Cin // group, *k)) * np.sqrt(2.0 / (Cin // group * k[0] * k[1]))).astype(np.float32)
        if exact16:
            x, w = _bc()._fp16_exact(x), _bc()._fp16_exact(w)
        return dict(x=x, w=w, b=rng.standard_normal(Cout).astype(np.float32))

    def setup(hip):
        kw = dict(plan_kw, **({"algo": getattr(hip, algo)} if algo else {}))
        plan = hip.ConvPlan(N, Cin, H, W, Cout, k[0], k[1], pad, stride, group, relu, **kw)
        assert kernel(plan.kernel) if callable(kernel) else plan.kernel == kernel, plan.kernel
        if split is not None:
            cls = plan.plan_class()
            assert cls["wino_gemm"] == 2 and bool(cls["wg_split"]) == bool(split), cls
        assert not pool or plan.can_pool
        return plan

    def run(hip, plan, b):
        plan.pack(b["w"])
        Ho, Wo = plan.out_shape()[2:]
        if plain:
            y = _empty(plan.out_shape())
            wsb = plan.ws.numel() * 4 if plan.ws is not None else 0
            hip._check(hip.lib().mscnn_conv2d_fwd_f32(plan._p, _vp(b["x"]), _vp(b["w"]), _vp(plan.packed), _vp(b["b"]), _vp(y), _vp(plan.ws),
                                                      wsb, hip._stream()))
            return [y]
        yp = _empty((N, Cout, (Ho + 1) // 2, (Wo + 1) // 2)) if pool else None
        y = plan.forward(b["x"], b["b"], pool_out=yp)
        return [y, yp] if pool else [y]

    def check(orc, i, o):
        r = orc.conv2d(i["x"], i["w"], None, pad, stride, group) + i["b"][None, :, None, None]
        r = np.maximum(r, 0) if relu else r
        _bc().finite(r)
        close(o[0], r)
        if pool:
            same(o[1], orc.pool2d(o[0], (2, 2), (0, 0), (2, 2), "MAX"))

    case(name, ("mscnn_conv2d_pack_weights", "mscnn_conv2d_fwd_f32" if plain else "mscnn_conv2d_fwd_pool_f32"), draw, run, check, setup=setup, workspaces=lambda plan: [plan.ws, plan.packed])


_is_igemm = lambda n: n.startswith("igemm_") and "_roi" not in n                                    # noqa: E731
_conv_case("conv_igemm_streamk", (1, 24, 36, 120, 256), _is_igemm, algo="ALGO_DIRECT")
_conv_case("conv_igemm_plain_entry", (2, 8, 10, 20, 130), _is_igemm, plain=True, algo="ALGO_DIRECT")
_conv_case("conv_igemm_fused_pool", (1, 8, 13, 37, 64), _is_igemm, pool=True, algo="ALGO_DIRECT")
_conv_case("conv_igemm_roi_mode", (13, 16, 7, 7, 256), lambda n: n.startswith("igemm_") and "_roi" in n, pad=(0, 0), algo="ALGO_DIRECT")
_conv_case("conv_igemm16", (1, 24, 13, 21, 64), lambda n: n.startswith("igemm16_"), exact16=True, algo="ALGO_F16")
_conv_case("conv_igemm16x3", (2, 32, 70, 130, 130), "igemm16x3_64x256_k3x3_tw32", relu_x=True, pool=True, algo="ALGO_WINO_F3_X3")
_conv_case("conv_head4x4", (1, 16, 12, 20, 7), lambda n: n.startswith("head4x4"), k=(5, 3), pad=(2, 1), relu=False, relu_x=True)
_conv_case("conv_head_kwfold", (1, 64, 36, 120, 9), lambda n: n.startswith("head_kwfold_shiftadd_f32"), k=(5, 5), pad=(2, 2), relu=False,
           relu_x=True, tune_flags=1024)
_conv_case("conv_head_gemm", (2, 64, 12, 20, 7), lambda n: n.startswith("head_gemm_shiftadd_f32"), k=(5, 3), pad=(2, 1), relu=False,
           relu_x=True, tune_flags=16)
_conv_case("conv_c3_valu", (1, 3, 130, 36, 16), "conv3x3_c3_valu_f32")
_conv_case("conv_wino_f2_one_launch", (3, 40, 24, 64, 64), "winograd2x2_fused_k3x3_c64", relu_x=True, pool=True, tune_variant=403)
_conv_case("conv_ring", (3, 40, 16, 128, 64), "wconv_64x512_k3x3", relu_x=True, pool=True, tune_variant=402, algo="ALGO_DIRECT")
_conv_case("conv_direct_f32", (2, 6, 9, 7, 4), "direct_f32", pad=(0, 0), stride=(2, 2), group=2)
_conv_case("conv_wino_f2", (1, 40, 13, 21, 130), "winograd_f2x2_3x3", algo="ALGO_WINO_F2")
_conv_case("conv_wino_f3_igemm_planes", (1, 40, 13, 21, 130), "winograd_f3x3_3x3", algo="ALGO_WINO_F3")
_conv_case("conv_wino_f4_igemm_planes", (1, 40, 13, 21, 130), "winograd_f4x4_3x3", pool=True, algo="ALGO_WINO_F4")
_conv_case("conv_wino_f3_wgemm_whole", (16, 32, 8, 4, 32), "winograd_f3x3_3x3", relu_x=True, split=0, algo="ALGO_WINO_F3")
_conv_case("conv_wino_f3_wgemm_split", (16, 32, 8, 4, 32), "winograd_f3x3_3x3", relu_x=True, split=1, algo="ALGO_WINO_F3", tune_variant=556)
_conv_case("conv_wino_f4_wgemm_whole", (1, 96, 24, 96, 64), "winograd_f4x4_3x3", pool=True, split=0, algo="ALGO_WINO_F4", tune_variant=812)
_conv_case("conv_wino_f4_wgemm_split", (1, 96, 24, 96, 64), "winograd_f4x4_3x3", pool=True, split=1, algo="ALGO_WINO_F4", tune_variant=556)
_conv_case("conv_wino_f3_x3", (2, 64, 10, 14, 32), "winograd_f3x3_3x3_x3f16_128", algo="ALGO_WINO_F3_X3", tune_flags=4)


def _chain_case():
    """Three chained F(4x4,3x3) layers (mscnn_conv2d_fwd_chain_f32), the shape of the buffer-contract case."""
    N, C0, C1, C2, H, W = 2, 8, 16, 24, 40, 200
    chans = [C0, C1, C2, C1]

    def draw(seed):
        rng = np.random.default_rng(seed)
        d = dict(x=rng.standard_normal((N, C0, H, W)).astype(np.float32))
        for i in range(3):
            d[f"w{i}"] = (rng.standard_normal((chans[i + 1], chans[i], 3, 3)) * np.sqrt(2.0 / (9 * chans[i]))).astype(np.float32)
            d[f"b{i}"] = rng.standard_normal(chans[i + 1]).astype(np.float32)
        return d

    def setup(hip):
        plans = [hip.ConvPlan(N, chans[i], H, W, chans[i + 1], 3, 3, (1, 1), relu=True, algo=hip.ALGO_WINO_F4) for i in range(3)]
        a, b, c = plans
        assert all(p.kernel == "winograd_f4x4_3x3" for p in plans) and a.can_chain(b) and b.can_chain(c) and c.can_pool_only
        return plans

    def run(hip, plans, bufs):
        a, b, c = plans
        for i, p in enumerate(plans):
            p.pack(bufs[f"w{i}"])
        a.forward_chain(bufs["x"], b, bufs["b0"], write_y=False)
        y2 = b.forward_chain(None, c, bufs["b1"], write_y=True)
        pool = _empty((N, chans[3], H // 2, W // 2))
        y3 = c.forward_chain(None, None, bufs["b2"], pool_out=pool)
        return [y2, y3, pool]

    def check(orc, i, o):
        r1 = orc.relu(orc.conv2d(i["x"], i["w0"], i["b0"], (1, 1)))
        r2 = orc.relu(orc.conv2d(r1, i["w1"], i["b1"], (1, 1)))
        r3 = orc.relu(orc.conv2d(r2, i["w2"], i["b2"], (1, 1)))
        _bc().finite(r1, r2, r3)
        close(o[0], r2)
        close(o[1], r3)
        same(o[2], orc.pool2d(o[1]))

    case("conv_chain_f4", ("mscnn_conv2d_pack_weights", "mscnn_conv2d_fwd_chain_f32"), draw, run, check, setup=setup,
         workspaces=lambda plans: [t for p in plans for t in (p.ws, p.packed)])


_chain_case()


def _roipool_fused_case():
    """Both ROI poolings fused into roi_c1's input stage, with the maps built inside the call and with prepared maps
    (mscnn_roipool_maps_build_f32), plus the unfused pair."""
    R, Cc, H8, W8, Cout, batch = 21, 64, 20, 28, 64, 2

    def draw(seed):
        rng = np.random.default_rng(seed)
        feat = np.maximum(rng.standard_normal((batch, Cc, H8, W8)), 0).astype(np.float32) * 3.0
        rois = _bc()._kitti_like_rois(rng, R, H8, W8, batch)
        w = (rng.standard_normal((Cout, 2 * Cc, 3, 3)) * np.sqrt(2.0 / (2 * Cc * 9))).astype(np.float32)
        return dict(feat=feat, rois=rois, w=w, b=rng.standard_normal(Cout).astype(np.float32))

    def setup(hip):
        plan = hip.ConvPlan(R, 2 * Cc, 7, 7, Cout, 3, 3, (0, 0), relu=True, algo=hip.ALGO_WINO_F3)
        assert plan.kernel == "winograd_f3x3_3x3" and plan.can_fuse_roipool(Cc, 7, 7)
        return plan

    def run(hip, plan, b):
        plan.pack(b["w"])
        y0 = plan.forward_roipool_pair(b["feat"], b["rois"], 0.125, 0.0, 0.25, b["b"])
        maps = hip.roipool_maps(b["feat"])
        y1 = plan.forward_roipool_pair(b["feat"], b["rois"], 0.125, 0.0, 0.25, b["b"], maps=maps)
        return [y0, y1, maps, hip.roipool_pair(b["feat"], b["rois"], 7, 7, 0.125, 0.0, 0.25)]

    def check(orc, i, o):
        pooled = np.concatenate([orc.roipool(i["feat"], i["rois"], 7, 7, 0.125, 0.0), orc.roipool(i["feat"], i["rois"], 7, 7, 0.125, 0.25)], 1)
        ref = orc.relu(orc.conv2d(pooled, i["w"], i["b"], (0, 0)))
        _bc().finite(pooled, ref)
        close(o[0], ref)
        close(o[1], ref)
        same(o[3], pooled)

    case("conv_roipool_pair_fused", ("mscnn_conv2d_pack_weights", "mscnn_conv2d_fwd_roipool_pair_f32", "mscnn_roipool_maps_build_f32",
                                     "mscnn_roipool_pair_fwd_f32"), draw, run, check, setup=setup,
         workspaces=lambda plan: [plan.ws, plan.packed])


_roipool_fused_case()


# ================================================================================================ inner product
def _ip_draw(M, N, K, exact16=False):
    def draw(seed):
        x, w, b, _ = _bc()._ip_data(M, N, K, seed, exact16=exact16)
        return dict(x=x, w=w, b=b)
    return draw


def _ip_check(relu=False, tol=1e-4):
    def check(orc, i, o):
        ref = i["x"].astype(np.float64) @ i["w"].astype(np.float64).T + i["b"]
        close(o[0], np.maximum(ref, 0) if relu else ref, tol)
    return check


for _name, _mnk in (("ip_generic", (5, 70, 33)), ("ip_mfma_streamk", (130, 192, 1000)), ("ip_rowwise", (676, 2, 4096))):
    case(_name, ("mscnn_inner_product_fwd_f32",), _ip_draw(*_mnk), lambda hip, s, b: [hip.inner_product(b["x"], b["w"], b["b"])], _ip_check())
case("ip_f16", ("mscnn_inner_product_pack_f16", "mscnn_inner_product_fwd_f16"), _ip_draw(257, 320, 1000, exact16=True),
     lambda hip, s, b: [hip.inner_product_f16(b["x"], b["w"], b["b"], relu=True)], _ip_check(relu=True))
case("ip_x3", ("mscnn_inner_product_x3_pack", "mscnn_inner_product_x3_fwd"), _ip_draw(33, 128, 96),
     lambda hip, s, b: [hip.inner_product_x3(b["x"], b["w"], b["b"], relu=True)], _ip_check(relu=True))


def _ip_wg_case():
    M, N, K = 193, 256, 64

    def setup(hip):
        assert hip.inner_product_wg_supported(M, N, K)
        wb = hip.lib().mscnn_inner_product_wg_workspace_bytes(M, N, K)
        return dict(wb=wb, ws=_empty((wb + 3) // 4), wt=_empty((K, N)))

    def run(hip, s, b):
        L = hip.lib()
        y = _empty((M, N))
        hip._check(L.mscnn_inner_product_wg_pack(_vp(b["w"]), _vp(s["wt"]), N, K, hip._stream()))
        hip._check(L.mscnn_inner_product_wg_fwd(_vp(b["x"]), _vp(s["wt"]), _vp(b["b"]), _vp(y), M, N, K, 1, _vp(s["ws"]), s["wb"], hip._stream()))
        return [y]

    case("ip_wg", ("mscnn_inner_product_wg_pack", "mscnn_inner_product_wg_fwd"), _ip_draw(M, N, K), run, _ip_check(relu=True), setup=setup,
         workspaces=lambda s: [s["ws"], s["wt"]])


_ip_wg_case()


# ================================================================================================ stock layers
def _std(shape, scale=1.0, names=("x",)):
    def draw(seed):
        rng = np.random.default_rng(seed)
        return {n: (rng.standard_normal(shape) * scale).astype(np.float32) for n in names}
    return draw


case("relu", ("mscnn_relu_fwd_f32",), _std(4099), lambda hip, s, b: [hip.relu(b["x"]), hip.relu(b["x"], 0.1)],
     lambda orc, i, o: (same(o[0], orc.relu(i["x"])), close(o[1], orc.relu(i["x"], 0.1), 1e-6)))
case("pool_fast_path", ("mscnn_pool2d_fwd_f32",), _std((1, 64, 32, 48)), lambda hip, s, b: [hip.pool2d(b["x"])],
     lambda orc, i, o: same(o[0], orc.pool2d(i["x"])))
case("pool_general", ("mscnn_pool2d_fwd_f32",), _std((1, 2, 7, 7)),
     lambda hip, s, b: [hip.pool2d(b["x"], (3, 3), (1, 1), (2, 2), "AVE"), hip.pool2d(b["x"], (3, 3), (2, 2), (2, 2), "MAX")],
     lambda orc, i, o: (close(o[0], orc.pool2d(i["x"], (3, 3), (1, 1), (2, 2), "AVE"), 1e-6),
                        same(o[1], orc.pool2d(i["x"], (3, 3), (2, 2), (2, 2), "MAX"))))
case("concat", ("mscnn_concat_channels_f32",),
     lambda seed: (lambda r: dict(a=r.standard_normal((5, 3, 7, 7)).astype(np.float32), b=r.standard_normal((5, 4, 7, 7)).astype(np.float32)))(
         np.random.default_rng(seed)),
     lambda hip, s, b: [hip.concat_channels([b["a"], b["b"]])], lambda orc, i, o: same(o[0], orc.concat_channels([i["a"], i["b"]])))


def _softmax_check(orc, i, o):
    x = i["x"].astype(np.float64)
    e = np.exp(x - x.max(1, keepdims=True))
    close(o[0], e / e.sum(1, keepdims=True), 1e-6)


case("softmax", ("mscnn_softmax_fwd_f32",), _std((2, 5, 3, 7), 3.0), lambda hip, s, b: [hip.softmax(b["x"])], _softmax_check)
case("eltwise", ("mscnn_eltwise_fwd_f32",), _std((37, 5), names=("a", "b", "c")),
     lambda hip, s, b: [hip.eltwise([b["a"], b["b"], b["c"]], op, cf) for op, cf in (("SUM", [0.33333333] * 3), ("PROD", None), ("MAX", None))],
     lambda orc, i, o: [same(o[j], orc.eltwise([i["a"], i["b"], i["c"]], op, cf))
                        for j, (op, cf) in enumerate((("SUM", [0.33333333] * 3), ("PROD", None), ("MAX", None)))])


def _deconv_cases():
    def draw(seed):
        rng = np.random.default_rng(seed)
        from oracle import pyoracle as orc
        return dict(x=np.maximum(rng.standard_normal((2, 8, 9, 11)), 0).astype(np.float32),
                    w=(orc.bilinear_filler((8, 1, 4, 4)) * rng.uniform(0.5, 1.5, (8, 1, 1, 1))).astype(np.float32),
                    b=rng.standard_normal(8).astype(np.float32), w3=rng.standard_normal((8, 1, 3, 3)).astype(np.float32))

    def check(orc, i, o):
        close(o[0], orc.deconv2d(i["x"], i["w"], i["b"], (1, 1), (2, 2), group=8), 1e-6)
        close(o[1], orc.deconv2d(i["x"], i["w3"], None, (1, 1), (1, 1), group=8), 1e-6)

    case("deconv_depthwise_quad_and_per_output", ("mscnn_deconv_depthwise_fwd_f32",), draw,
         lambda hip, s, b: [hip.deconv_depthwise(b["x"], b["w"], b["b"], (1, 1), (2, 2)), hip.deconv_depthwise(b["x"], b["w3"], None, (1, 1), (1, 1))],
         check)

    def draw_g(seed):
        rng = np.random.default_rng(seed)
        return dict(x=rng.standard_normal((2, 6, 5, 7)).astype(np.float32), w=(rng.standard_normal((6, 2, 3, 3)) * 0.3).astype(np.float32),
                    b=rng.standard_normal(4).astype(np.float32))

    def run_g(hip, s, b):
        y = _empty((2, 4, 9, 13))
        _bc()._deconv2d(hip, b["x"], b["w"], b["b"], y, 4, (1, 1), (2, 2), 2)
        return [y]

    case("deconv_generic", ("mscnn_deconv2d_fwd_f32",), draw_g, run_g,
         lambda orc, i, o: close(o[0], orc.deconv2d(i["x"], i["w"], i["b"], (1, 1), (2, 2), group=2)))


_deconv_cases()


def _metric_case():
    def draw(seed):
        rng = np.random.default_rng(seed)
        ref = (rng.standard_normal((5, 19, 33)) * 7).astype(np.float32)
        return dict(a=(ref + rng.standard_normal(ref.shape).astype(np.float32) * 1e-3).astype(np.float32), ref=ref)

    def run(hip, s, b):
        ss = hip.sum_squares(b["ref"])
        buf = _zeros(8, _torch().int32)
        hip.store_words(buf[2:], [11, -3, 2 ** 31 - 1])
        return [ss, hip.max_rel_diff(b["a"], b["ref"]), hip.max_rel_diff_strided(b["a"], 19 * 33, b["ref"], 19 * 33, 5, 19 * 33, ss, 5 * 19 * 33), buf]

    def check(orc, i, o):
        a, ref = i["a"].astype(np.float64), i["ref"].astype(np.float64)
        ss = float((ref ** 2).sum())
        assert abs(float(o[0][0]) - ss) <= 1e-9 * ss
        want = (np.abs(a - ref) / np.maximum(1.0, np.abs(ref))).max()
        assert abs(float(o[1][0]) - want) <= 1e-6 * want
        w2 = (np.abs(a - ref) / np.maximum(max(1.0, np.sqrt((ref ** 2).mean())), np.abs(ref))).max()
        assert abs(float(o[2][0]) - w2) <= 1e-5 * w2
        assert o[3].tolist() == [0, 0, 11, -3, 2 ** 31 - 1, 0, 0, 0]

    # output 0: sum_squares adds one f64 partial sum per wave with atomicAdd, in the order the waves finish -- not bit-reproducible
    # from run to run on any stream; its bar is the 1e-9 of check()
    case("metrics_and_store_words", ("mscnn_sum_squares_f32", "mscnn_max_rel_diff_f32", "mscnn_max_rel_diff_strided_f32", "mscnn_store_words_i32"),
         draw, run, check, unordered=(0,))


_metric_case()


# ================================================================================================ ROI ops
def _roi_draw(Cc=24, H=36, W=120, R=97, scale=0.125):
    def draw(seed):
        rng = np.random.default_rng(seed)
        return dict(feat=rng.standard_normal((2, Cc, H, W)).astype(np.float32), rois=_bc()._roi_set(rng, R, scale, H, W))
    return draw


case("roipool", ("mscnn_roipool_fwd_f32",), _roi_draw(), lambda hip, s, b: [hip.roipool(b["feat"], b["rois"], 7, 7, 0.125, 0.25)],
     lambda orc, i, o: same(o[0], orc.roipool(i["feat"], i["rois"], 7, 7, 0.125, 0.25)))
case("roipool_pair", ("mscnn_roipool_pair_fwd_f32",), _roi_draw(40, 36, 150, 33, 0.25),
     lambda hip, s, b: [hip.roipool_pair(b["feat"], b["rois"], 7, 5, 0.25, 0.0, 0.25)],
     lambda orc, i, o: (same(o[0][:, :40], orc.roipool(i["feat"], i["rois"], 7, 5, 0.25, 0.0)),
                        same(o[0][:, 40:], orc.roipool(i["feat"], i["rois"], 7, 5, 0.25, 0.25))))
case("roialign", ("mscnn_roialign_fwd_f32",), _roi_draw(), lambda hip, s, b: [hip.roialign(b["feat"], b["rois"], 7, 7, 0.125, 0.25)],
     lambda orc, i, o: same(o[0], orc.roialign(i["feat"], i["rois"], 7, 7, 0.125, 0.25)))


def _ave(orc, i, pad):
    return orc.pool2d(orc.roialign(i["feat"], i["rois"], 7, 7, 0.125, pad), (2, 2), (0, 0), (1, 1), "AVE")


# (the bar of tests/test_gpu_roialign_pair.py: the one-pass ops against the oracle's ROIAlign -> AVE pooling -> Concat, 1e-6)
case("roialign_ave", ("mscnn_roialign_ave_fwd_f32",), _roi_draw(), lambda hip, s, b: [hip.roialign_ave(b["feat"], b["rois"], 7, 7, 0.125, 0.25)],
     lambda orc, i, o: close(o[0], _ave(orc, i, 0.25), 1e-6))
case("roialign_ave_pair", ("mscnn_roialign_ave_pair_fwd_f32",), _roi_draw(),
     lambda hip, s, b: [hip.roialign_ave_pair(b["feat"], b["rois"], 7, 7, 0.125, 0.0, 0.25)],
     lambda orc, i, o: close(o[0], orc.concat_channels([_ave(orc, i, 0.0), _ave(orc, i, 0.25)]), 1e-6))


def _ingest_case():
    """mscnn_rois_ingest_f32 on net-coordinate rows grouped by image: float32 [image x1 y1 x2 y2 score]."""
    R, Nimg = 37, 2

    def draw(seed):
        rng = np.random.default_rng(seed)
        r = _bc()._random_rois(rng, R, 576, 1920, batch=Nimg)
        r = r[np.argsort(r[:, 0], kind="stable")]
        return dict(rows=np.concatenate([r, rng.standard_normal((R, 1)).astype(np.float32)], 1).astype(np.float32))

    def run(hip, s, b):
        torch = _torch()
        rois, props = _empty((R, 5)), _empty((R, 6))
        image_rows, status = torch.full((Nimg,), -1, dtype=torch.int32, device="cuda"), torch.full((4,), -1, dtype=torch.int32, device="cuda")
        hip._check(hip.lib().mscnn_rois_ingest_f32(_vp(b["rows"]), hip.ROIS_NET, R, Nimg, None, None, _vp(rois), _vp(props), _vp(image_rows),
                                                   _vp(status), hip._stream()))
        return [rois, props, image_rows, status]

    def check(orc, i, o):
        rows = i["rows"]
        assert o[3].tolist() == [1, -1, 0, 0], o[3]                 # accepted (tests/test_gpu_forward_rois.py)
        same(o[0], rows[:, :5])
        same(o[1], rows)
        assert o[2].tolist() == [int((rows[:, 0] == n).sum()) for n in range(Nimg)]

    case("rois_ingest", ("mscnn_rois_ingest_f32",), draw, run, check)


_ingest_case()


# ================================================================================================ pre-processing
def _preprocess_cases():
    orgs = [(96, 130), (50, 41), (33, 200)]
    H, W = 40, 57
    mean = (104.0, 117.0, 123.0)

    def draw(seed):
        return {f"f{j}": _bc()._rgb(h, w, 100 * seed + j) for j, (h, w) in enumerate(orgs)}

    def setup(hip):
        L = hip.lib()
        L.mscnn_preprocess_workspace_bytes.restype = C.c_size_t
        L.mscnn_preprocess_batch_workspace_bytes.restype = C.c_size_t
        L.mscnn_preprocess_batch_workspace_bytes.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        torch = _torch()
        B = len(orgs)
        oh, ow = (C.c_int * B)(*[h for h, _ in orgs]), (C.c_int * B)(*[w for _, w in orgs])
        views = [dict(frame=0, x0=3, y0=5, w=100, h=70), dict(frame=1, x0=0, y0=0, w=41, h=50, flip_x=1), dict(frame=2, x0=20, y0=1, w=64, h=32)]
        va = hip.view_array(views)
        wb1 = L.mscnn_preprocess_workspace_bytes(orgs[0][0], orgs[0][1], H, W)
        wbB = L.mscnn_preprocess_batch_workspace_bytes(B, oh, ow, H, W)
        wbV = L.mscnn_preprocess_views_workspace_bytes(va, len(views), H, W)
        mk = lambda n: torch.empty(max(n, 1), dtype=torch.uint8, device="cuda")      # noqa: E731
        return dict(oh=oh, ow=ow, va=va, views=views, wb=(wb1, wbB, wbV), ws=(mk(wb1), mk(wbB), mk(wbV)), m=(C.c_float * 3)(*mean))

    def run(hip, s, b):
        L = hip.lib()
        B = len(orgs)
        fr = [b[f"f{j}"] for j in range(B)]
        ptrs = (C.c_void_p * B)(*[f.data_ptr() for f in fr])
        o1, oB, oV = _empty((1, 3, H, W)), _empty((B, 3, H, W)), _empty((len(s["views"]), 3, H, W))
        hip._check(L.mscnn_preprocess_u8_f32(_vp(fr[0]), orgs[0][0], orgs[0][1], _vp(o1), H, W, s["m"], _vp(s["ws"][0]), C.c_size_t(s["wb"][0]),
                                             hip._stream()))
        hip._check(L.mscnn_preprocess_batch_u8_f32(ptrs, s["oh"], s["ow"], B, _vp(oB), H, W, s["m"], _vp(s["ws"][1]), C.c_size_t(s["wb"][1]),
                                                   hip._stream()))
        hip._check(L.mscnn_preprocess_views_u8_f32(ptrs, s["oh"], s["ow"], B, s["va"], len(s["views"]), _vp(oV), H, W, s["m"], _vp(s["ws"][2]),
                                                   C.c_size_t(s["ws"][2].numel()), hip._stream()))
        return [o1, oB, oV]

    def check(orc, i, o):
        fr = [i[f"f{j}"] for j in range(len(orgs))]
        same(o[0], orc.preprocess(fr[0], H, W))
        same(o[1], np.concatenate([orc.preprocess(f, H, W) for f in fr], 0))
        wins = []
        for v in ({**dict(flip_x=0), **v} for v in [dict(frame=0, x0=3, y0=5, w=100, h=70), dict(frame=1, x0=0, y0=0, w=41, h=50, flip_x=1),
                                                     dict(frame=2, x0=20, y0=1, w=64, h=32)]):
            win = fr[v["frame"]][v["y0"]:v["y0"] + v["h"], v["x0"]:v["x0"] + v["w"]]
            wins.append(orc.preprocess(np.ascontiguousarray(win[:, ::-1] if v["flip_x"] else win), H, W))
        same(o[2], np.concatenate(wins, 0))

    case("preprocess_single_batch_views", ("mscnn_preprocess_u8_f32", "mscnn_preprocess_batch_u8_f32", "mscnn_preprocess_views_u8_f32"),
         draw, run, check, setup=setup, workspaces=lambda s: list(s["ws"]))


_preprocess_cases()


# ================================================================================================ proposals
for _n in (65, 4033):
    case(f"nms_greedy_{_n}", ("mscnn_nms_greedy_f32",), (lambda n: lambda seed: dict(boxes=_bc()._clustered_boxes(np.random.default_rng(seed), n)))(_n),
         lambda hip, s, b: [hip.nms_greedy(b["boxes"], 0.65, "IOU")],
         lambda orc, i, o: (same(o[0], orc.nms_greedy(i["boxes"], 0.65, "IOU")), None))


def _decode_draw(seed):
    rng = np.random.default_rng(seed)
    return dict(prior=_bc()._random_rois(rng, 37, 576, 1920), bbox=rng.standard_normal((37, 8)).astype(np.float32))


case("decodebbox", ("mscnn_decodebbox_fwd_f32",), _decode_draw,
     lambda hip, s, b: [hip.decode_bbox(b["bbox"], b["prior"], (0, 0, 0, 0), (0.1, 0.1, 0.2, 0.2))],
     lambda orc, i, o: same(o[0], orc.decode_bbox(i["bbox"], i["prior"], (0, 0, 0, 0), (0.1, 0.1, 0.2, 0.2))))

BO_KW = dict(fg_thr=-5.0, iou_thr=0.65, max_nms_num=2000, min_size=15.0)


def _boxoutput_case(name, abi, one_pass, num):
    def draw(seed):
        bc = _bc()
        return {f"h{j}": h for j, h in enumerate(bc._heads(np.random.default_rng(seed), bc.KITTI_HEADS["shapes"], num=num, bg_bias=-8.0))}

    def setup(hip):
        K = _bc().KITTI_HEADS
        return hip.BoxOutput(hip.make_boxoutput_desc(K["shapes"], num, 9, K["field"], K["field"], K["ds"], **BO_KW), one_pass=one_pass)

    def run(hip, layer, b):
        for t in (layer.rois, layer.props, layer.aids):      # rows past the count are not the op's to write: zeros in every run
            t.zero_()
        layer.forward_async([b[f"h{j}"] for j in range(len(b))])
        return [layer.count, layer.rois, layer.props, layer.aids]

    def check(orc, i, o):
        K = _bc().KITTI_HEADS
        rois_r, props_r, _, nreal_r, aids_r = orc.boxoutput([i[f"h{j}"] for j in range(len(i))], K["field"], K["field"], K["ds"],
                                                            with_anchor_ids=True, **BO_KW)
        R, nreal = o[0].tolist()
        assert nreal == nreal_r and nreal_r > 100
        same(o[1][:R], rois_r)
        same(o[2][:R], props_r)
        same(o[3][:R], aids_r)

    case(name, abi, draw, run, check, setup=setup, workspaces=lambda layer: [layer.ws])


_boxoutput_case("boxoutput_single", ("mscnn_boxoutput_fwd_f32",), False, 1)
_boxoutput_case("boxoutput_batch", ("mscnn_boxoutput_batch_fwd_f32",), True, 2)


# ================================================================================================ final stage
FINAL_KW = dict(cls_id=2, ratios=(576 / 375, 1920 / 1242), org_hw=(375, 1242))


def _final_case(name, fn, cascade, nms, R=37):
    """The single-list final stages on the C ABI (the wrappers read the count back).  dets, ids and the count start as zeros on the
    call's stream, so rows past the count are zeros in every run."""
    def draw(seed):
        a, b, c = (_bc()._cascade_inputs if cascade else _bc()._final_inputs)(R, seed)
        return dict(a=a, b=b, props=c)

    def setup(hip):
        torch = _torch()
        wb = hip.lib().mscnn_detections_workspace_bytes(R)
        return dict(wb=wb, ws=torch.empty(wb, dtype=torch.uint8, device="cuda"))

    def run(hip, s, b):
        torch = _torch()
        d = hip.DetectionsDesc()
        hip._fill_desc(d, b["b"].shape[1], FINAL_KW)
        dets, ids, count = _zeros((R, 5), torch.float64), _zeros(R, torch.int32), _zeros(1, torch.int32)
        f = getattr(hip.lib(), fn)
        head = [C.byref(d)] + ([C.c_float(0.2)] if cascade else []) + ([hip._nms_ref(nms)] if nms is not None else [])
        hip._check(f(*head, _vp(b["a"]), _vp(b["b"]), _vp(b["props"]), R, _vp(dets), _vp(ids), _vp(count), _vp(s["ws"]), C.c_size_t(s["wb"]),
                     hip._stream()))
        return [count, dets, ids]

    def check(orc, i, o):
        kw = dict(FINAL_KW, **(dict(det_thr=0.2) if cascade else {}))
        dref, iref = (orc.detections_cascade if cascade else orc.detections)(i["a"], i["b"], i["props"], **kw)
        D = int(o[0][0])
        assert D == len(iref) and D > 0
        same(o[2][:D], iref)
        (same if cascade else close)(o[1][:D], dref)

    case(name, (fn,), draw, run, check, setup=setup, workspaces=lambda s: [s["ws"]])


_NMS_DEFAULT = {}      # nms_params() without arguments: bbNms's defaults, the setting of the calls without the struct -- the oracle's
_final_case("detections_plain", "mscnn_detections_fwd", False, None)
_final_case("detections_plain_nms", "mscnn_detections_nms_fwd", False, _NMS_DEFAULT)
_final_case("detections_cascade", "mscnn_detections_cascade_fwd", True, None)
_final_case("detections_cascade_nms", "mscnn_detections_cascade_nms_fwd", True, _NMS_DEFAULT)


def multi_inputs(seed, cascade):
    """The two-image inputs of the buffer-contract file's multi cases (63 + 40 resp. 40 + 64 rows)."""
    bc = _bc()
    rows = [40, 64] if cascade else [63, 40]
    parts = []
    for i, n in enumerate(rows):
        a, b, pr = (bc._cascade_inputs if cascade else bc._final_inputs)(n, 10 * seed + i)
        pr[:, 0] = i
        if cascade:
            a[:, 0] = i
        else:
            a, b = a[:, :16], b[:, :4]
        parts.append((a, b, pr))
    a, b, props = (np.ascontiguousarray(np.concatenate([p[j] for p in parts], 0)) for j in range(3))
    return rows, dict(a=a, b=b, props=props)


def multi_segments(cascade):
    return [dict(cls_id=c, **_bc()._image_kw(i, 0.4 if cascade else 0.6)) for i in range(2) for c in (2, 3)]


def multi_state(hip, cascade, R=103, M=64):
    torch = _torch()
    segs = multi_segments(cascade)
    S = len(segs)
    cap = 2 * R
    f = hip.lib().mscnn_detections_cascade_multi_workspace_bytes if cascade else hip.lib().mscnn_detections_multi_workspace_bytes
    wb = f(S, M)
    return dict(S=S, cap=cap, wb=wb, M=M, R=R, segs=segs, ws=torch.empty(max(wb, 1), dtype=torch.uint8, device="cuda"),
                pack_bytes=hip.lib().mscnn_detections_multi_pack_bytes(S, cap))


def multi_run(hip, s, b, cascade, nms=None):
    """mscnn_detections_multi_fwd / _cascade_multi_fwd (or their _nms forms) into a pack zero-filled on the call's stream."""
    torch = _torch()
    L = hip.lib()
    S, R, M, cap = s["S"], s["R"], s["M"], s["cap"]
    pack = torch.zeros(s["pack_bytes"], dtype=torch.uint8, device="cuda")
    descs = (hip.DetectionsDesc * S)()
    ncls = b["b"].shape[1]
    for k, kw in enumerate(s["segs"]):
        hip._fill_desc(descs[k], ncls, kw)
    if cascade:
        outs = (hip.CascadeOutput * 1)()
        outs[0].boxes, outs[0].cls_prob, outs[0].props, outs[0].ncls = b["a"].data_ptr(), b["b"].data_ptr(), b["props"].data_ptr(), ncls
        if nms is None:
            hip._check(L.mscnn_detections_cascade_multi_fwd(descs, C.c_float(0.25), 2, 1, 2, outs, R, M, _vp(pack), cap, _vp(s["ws"]),
                                                            C.c_size_t(s["wb"]), hip._stream()))
        else:
            hip._check(L.mscnn_detections_cascade_multi_nms_fwd(descs, C.c_float(0.25), hip._nms_ref(nms), 2, 1, 2, outs, R, M, _vp(pack), cap,
                                                                _vp(s["ws"]), C.c_size_t(s["wb"]), hip._stream()))
    elif nms is None:
        hip._check(L.mscnn_detections_multi_fwd(descs, 2, 2, _vp(b["a"]), _vp(b["b"]), _vp(b["props"]), R, M, _vp(pack), cap, _vp(s["ws"]),
                                                C.c_size_t(s["wb"]), hip._stream()))
    else:
        hip._check(L.mscnn_detections_multi_nms_fwd(descs, hip._nms_ref(nms), 2, 2, _vp(b["a"]), _vp(b["b"]), _vp(b["props"]), R, M, _vp(pack), cap,
                                                    _vp(s["ws"]), C.c_size_t(s["wb"]), hip._stream()))
    return [pack]


def multi_check(hip, orc, i, pack, cascade, R=103):
    rows = [40, 64] if cascade else [63, 40]
    segs = multi_segments(cascade)
    out = hip._read_multi_pack(_torch().from_numpy(pack), len(segs), 2, R, 2 * R, "multi")
    some = False
    for s, (dets, ids, row0, n) in enumerate(out):
        im = s // 2
        sl = slice(sum(rows[:im]), sum(rows[:im + 1]))
        assert (row0, n) == (sl.start, rows[im])
        if cascade:
            dref, iref = orc.detections_cascade(i["a"][sl], i["b"][sl], i["props"][sl], det_thr=0.25, **segs[s])
        else:
            dref, iref = orc.detections(i["a"][sl], i["b"][sl], i["props"][sl], **segs[s])
        same(ids, iref)
        (same if cascade else close)(dets, dref)
        some = some or len(iref) > 0
    assert some


def _multi_case(name, fn, cascade, nms):
    R = 104 if cascade else 103

    def setup(hip):
        return multi_state(hip, cascade, R=R)
    holder = {}

    def run(hip, s, b):
        holder["hip"] = hip
        return multi_run(hip, s, b, cascade, nms)

    case(name, (fn,), lambda seed: multi_inputs(seed, cascade)[1], run,
         lambda orc, i, o: multi_check(holder["hip"], orc, i, o[0], cascade, R=R), setup=setup, workspaces=lambda s: [s["ws"]])


_multi_case("detections_multi", "mscnn_detections_multi_fwd", False, None)
_multi_case("detections_multi_nms", "mscnn_detections_multi_nms_fwd", False, _NMS_DEFAULT)
_multi_case("detections_cascade_multi", "mscnn_detections_cascade_multi_fwd", True, None)
_multi_case("detections_cascade_multi_nms", "mscnn_detections_cascade_multi_nms_fwd", True, _NMS_DEFAULT)


# ================================================================================================ video: proposals
def _proposals_case():
    counts = [65, 0, 130]

    def draw(seed):
        from proposals_witness import synth_props
        return dict(props=synth_props(counts, seed))

    def images():
        from proposals_witness import RATIOS
        return [dict(ratios=RATIOS[i % len(RATIOS)]) for i in range(len(counts))]

    holder = {}

    def run(hip, s, b):
        torch = _torch()
        holder["hip"] = hip
        R, B = sum(counts), len(counts)
        descs = (hip.ProposalsDesc * B)()
        for i, kw in enumerate(images()):
            descs[i].proposal_thr = -10.0
            descs[i].ratio_h, descs[i].ratio_w = kw["ratios"]
        pack = torch.zeros(hip.lib().mscnn_proposals_multi_pack_bytes(B, R), dtype=torch.uint8, device="cuda")
        hip._check(hip.lib().mscnn_proposals_multi_fwd(descs, B, _vp(b["props"]), R, _vp(pack), R, hip._stream()))
        return [pack]

    def check(orc, i, o):
        from proposals_witness import batch_witness
        hip = holder["hip"]
        R = sum(counts)
        out = hip._read_multi_pack(_torch().from_numpy(o[0]), len(counts), 1, R, R, "proposals_multi")
        for (p, rows, row0, n), (wp, wk, wrow0, wn) in zip(out, batch_witness(i["props"], images())):
            assert (row0, n) == (wrow0, wn)
            assert p.shape == wp.shape and np.array_equal(p.view(np.uint64), np.ascontiguousarray(wp, np.float64).view(np.uint64))
            same(rows, wk)

    case("proposals_multi", ("mscnn_proposals_multi_fwd",), draw, run, check)


_proposals_case()


# ================================================================================================ merge
# Two forwards of two images and two classes (test_gpu_soft's "S4_two_passes": every row is a candidate; the second forward is
# mirrored and at other ratios), 200 slots per list.  run(): candidates_reset, the first forward through candidates_add, the second
# through candidates_add_views with the identity frame mapping, then one merge op into a 0xFF pack made on the call's stream.  The
# bar is each op's own: the pack byte for byte as its witness says (tests/test_gpu_soft.py, _matrix, _wbf, _seq, _vote).
MERGE_CAP, MERGE_CLASSES, SEED = 200, [2, 3], 1701
_merge_cache = {}


def _merge_passes(seed):
    if seed not in _merge_cache:
        import test_gpu_soft as gs
        passes = [gs.Pass(0, [65, 64], seed=seed), gs.Pass(1, [63, 66], ratios=(1.5, 1.25), view=gs.FLIP, seed=seed)]
        _merge_cache[seed] = (passes, gs.lists_of(passes, MERGE_CLASSES))
    return _merge_cache[seed]


def _merge_draw(seed):
    passes, _ = _merge_passes(seed)
    return {f"{n}{k}": getattr(p, a) for k, p in enumerate(passes) for n, a in (("bbox", "bbox_pred"), ("cls", "cls_pred"), ("props", "props"))}


def _merge_setup(ws_bytes):
    def setup(hip):
        torch = _torch()
        L = hip.lib()
        S = 2 * len(MERGE_CLASSES)
        return dict(S=S, buf=torch.empty(L.mscnn_detections_candidates_bytes(S, MERGE_CAP), dtype=torch.uint8, device="cuda"),
                    ws=torch.empty(max(ws_bytes(L, S), 1), dtype=torch.uint8, device="cuda"),
                    nbytes=L.mscnn_detections_multi_pack_bytes(S, S * MERGE_CAP))
    return setup


def _merge_fill(hip, s, b):
    """reset + the two adds, on the current stream; returns the 0xFF pack."""
    torch = _torch()
    L = hip.lib()
    passes, _ = _merge_passes(SEED)                                   # (the shapes, ratios and views: the same for every seed)
    S, K = s["S"], len(MERGE_CLASSES)
    hip._check(L.mscnn_detections_candidates_reset(_vp(s["buf"]), S, MERGE_CAP, hip._stream()))
    for k, p in enumerate(passes):
        descs = (hip.DetectionsDesc * S)()
        for j in range(S):
            hip._fill_desc(descs[j], p.ncls, p.seg_kw(MERGE_CLASSES[j % K]))
        views = hip._view_array(None if p.view is None else [p.view] * 2, 2)
        args = (k, 2, K, _vp(b[f"bbox{k}"]), _vp(b[f"cls{k}"]), _vp(b[f"props{k}"]), b[f"props{k}"].shape[0], _vp(s["buf"]), MERGE_CAP, hip._stream())
        if k == 0:
            hip._check(L.mscnn_detections_candidates_add(descs, views, None, *args))
        else:
            hip._check(L.mscnn_detections_candidates_add_views(descs, views, (C.c_int * 2)(0, 1), None, k, 2, S // K, *args[2:]))
    return torch.full((s["nbytes"],), 0xFF, dtype=torch.uint8, device="cuda")


def _ov(S):
    import test_gpu_soft as gs
    return (C.c_double * S)(*[gs.OVERLAP] * S)


def _merge_expected(nbytes, segment):
    """The 0xFF pack with, per list, what segment(lists of the list) -> (dets, pass, row) says."""
    import test_gpu_soft as gs
    _, lists = _merge_passes(SEED)
    S = len(lists)
    want = np.full(nbytes, 0xFF, np.uint8)
    hdr, dets, tags = gs.pack_views(want, S, MERGE_CAP)
    hdr[0] = [S, MERGE_CAP, S * MERGE_CAP, 0]
    for s, l in enumerate(lists):
        d, pas, row = segment(l)
        hdr[1 + s] = [len(d), sum(len(r) for r, _ in l), s * MERGE_CAP, 0]
        dets[s * MERGE_CAP:s * MERGE_CAP + len(d)] = d
        tags[s * MERGE_CAP:s * MERGE_CAP + len(d)] = (np.asarray(pas).astype(np.int32) << 24) | row
    assert hdr[1:, 0].max() > 5
    return want


def _same_bytes(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]


def _merge_cases():
    import_gs = lambda: __import__("test_gpu_soft")      # noqa: E731

    # ---- hard NMS, and the vote behind it
    def run_plain(vote):
        def run(hip, s, b):
            pack = _merge_fill(hip, s, b)
            hip._check(hip.lib().mscnn_detections_merge_fwd(_ov(s["S"]), None, s["S"], _vp(s["buf"]), MERGE_CAP, _vp(pack), _vp(s["ws"]),
                                                            C.c_size_t(s["ws"].numel()), hip._stream()))
            if vote:
                hip._check(hip.lib().mscnn_detections_merge_vote_fwd(C.byref(hip.VoteParams(0.5)), s["S"], _vp(s["buf"]), MERGE_CAP, _vp(pack),
                                                                     hip._stream()))
            return [pack]
        return run

    def check_plain(orc, i, o):
        import merge_witness as mw
        gs = import_gs()
        _same_bytes(o[0], _merge_expected(len(o[0]), lambda l: mw.merge(l, gs.OVERLAP, "maxg", "union")[:3]))

    def check_vote(orc, i, o):
        import vote_witness as vw
        moved = []

        def seg(l):
            d, voted, pas, row, _, who, _ = vw.vote_segment(l, 0.5, overlap=import_gs().OVERLAP)
            moved.append(int(np.count_nonzero(np.any(voted[:, :4] != d[:, :4], 1))))
            return voted, pas, row
        _same_bytes(o[0], _merge_expected(len(o[0]), seg))
        assert sum(moved) > 0, "the vote moved no box: the case shows nothing"

    ws_merge = lambda L, S: L.mscnn_detections_merge_workspace_bytes(S, MERGE_CAP)      # noqa: E731
    case("merge_hard_nms", ("mscnn_detections_candidates_reset", "mscnn_detections_candidates_add", "mscnn_detections_candidates_add_views",
                            "mscnn_detections_merge_fwd"), _merge_draw, run_plain(False), check_plain, setup=_merge_setup(ws_merge),
         workspaces=lambda s: [s["ws"]], seed=SEED)
    case("merge_vote", ("mscnn_detections_merge_fwd", "mscnn_detections_merge_vote_fwd"), _merge_draw, run_plain(True), check_vote,
         setup=_merge_setup(ws_merge), workspaces=lambda s: [s["ws"]], seed=SEED)

    # ---- Soft-NMS (linear: bit-exact against the witness)
    def run_soft(hip, s, b):
        pack = _merge_fill(hip, s, b)
        soft = hip.SoftNmsParams(hip.soft_nms_method("linear"), 0.5, 0.05, 0)
        hip._check(hip.lib().mscnn_detections_merge_soft_fwd(_ov(s["S"]), C.byref(soft), s["S"], _vp(s["buf"]), MERGE_CAP, _vp(pack), _vp(s["ws"]),
                                                             C.c_size_t(s["ws"].numel()), hip._stream()))
        return [pack]

    def check_soft(orc, i, o):
        gs = import_gs()
        want, _ = gs.expected_pack(len(o[0]), _merge_passes(SEED)[1], MERGE_CAP, "linear", score_thr=0.05, max_out=0)
        _same_bytes(o[0], want)

    case("merge_soft", ("mscnn_detections_merge_soft_fwd",), _merge_draw, run_soft, check_soft,
         setup=_merge_setup(lambda L, S: L.mscnn_detections_merge_soft_workspace_bytes(S, MERGE_CAP)), workspaces=lambda s: [s["ws"]], seed=SEED)

    # ---- Matrix NMS (linear)
    def run_matrix(hip, s, b):
        pack = _merge_fill(hip, s, b)
        mx = hip.MatrixNmsParams(hip.matrix_nms_method("linear"), 0.5, 0.05, 0)
        hip._check(hip.lib().mscnn_detections_merge_matrix_fwd(C.byref(mx), s["S"], _vp(s["buf"]), MERGE_CAP, _vp(pack), _vp(s["ws"]),
                                                               C.c_size_t(s["ws"].numel()), hip._stream()))
        return [pack]

    def check_matrix(orc, i, o):
        import test_gpu_matrix as gm
        want, _ = gm.expected_pack(len(o[0]), _merge_passes(SEED)[1], MERGE_CAP, "linear", score_thr=0.05)
        _same_bytes(o[0], want)

    case("merge_matrix", ("mscnn_detections_merge_matrix_fwd",), _merge_draw, run_matrix, check_matrix,
         setup=_merge_setup(lambda L, S: L.mscnn_detections_merge_matrix_workspace_bytes(S, MERGE_CAP)), workspaces=lambda s: [s["ws"]], seed=SEED)

    # ---- weighted boxes fusion
    def run_wbf(hip, s, b):
        torch = _torch()
        pack = _merge_fill(hip, s, b)
        members = torch.full((s["S"] * MERGE_CAP,), -1, dtype=torch.int32, device="cuda")
        wbf = hip.WbfParams(0.55, 0.05, hip.wbf_conf_type("avg"), 0)
        hip._check(hip.lib().mscnn_detections_merge_wbf_fwd(C.byref(wbf), (C.c_int * s["S"])(*[2] * s["S"]), s["S"], _vp(s["buf"]), MERGE_CAP, _vp(pack),
                                                            _vp(members), _vp(s["ws"]), C.c_size_t(s["ws"].numel()), hip._stream()))
        return [pack, members]

    def check_wbf(orc, i, o):
        import test_gpu_wbf as gw
        import wbf_witness as ww
        want, wmem, _ = gw.expected_of(len(o[0]), _merge_passes(SEED)[1], MERGE_CAP, expected=2, thr=0.55, skip_thr=0.05,
                                       conf_type=ww.CONF_TYPES["avg"], max_out=0)
        _same_bytes(o[0], want)
        _same_bytes(o[1], wmem)

    case("merge_wbf", ("mscnn_detections_merge_wbf_fwd",), _merge_draw, run_wbf, check_wbf,
         setup=_merge_setup(lambda L, S: L.mscnn_detections_merge_wbf_workspace_bytes(S, MERGE_CAP)), workspaces=lambda s: [s["ws"]], seed=SEED)

    # ---- Seq-NMS: the two images as the two frames of a clip (list = frame x 2 + class)
    def run_seq(hip, s, b):
        torch = _torch()
        pack = _merge_fill(hip, s, b)
        seq = torch.full((s["S"] * MERGE_CAP,), -1, dtype=torch.int32, device="cuda")
        sq = hip.SeqNmsParams(0.5, 0.05, 300, hip.seq_nms_rescore("avg"), 0)
        hip._check(hip.lib().mscnn_detections_merge_seq_fwd(_ov(s["S"]), C.byref(sq), 2, s["S"] // 2, _vp(s["buf"]), MERGE_CAP, _vp(pack), _vp(seq),
                                                            _vp(s["ws"]), C.c_size_t(s["ws"].numel()), hip._stream()))
        return [pack, seq]

    def check_seq(orc, i, o):
        import seq_cases
        want, wseq, _, _ = seq_cases.expected_of(len(o[0]), _merge_passes(SEED)[1], 2, MERGE_CAP, score_thr=0.05)
        _same_bytes(o[0], want)
        _same_bytes(o[1], wseq)

    case("merge_seq", ("mscnn_detections_merge_seq_fwd",), _merge_draw, run_seq, check_seq,
         setup=_merge_setup(lambda L, S: L.mscnn_detections_merge_seq_workspace_bytes(2, S // 2, MERGE_CAP, 300)), workspaces=lambda s: [s["ws"]],
         seed=SEED)


_merge_cases()


def _cascade_merge_case():
    """Two cascade forwards (test_gpu_detect_merge.cascade_pass: two outputs, rows [64, 33], class 2; the second mirrored at other
    ratios): the first through candidates_cascade_add, the second through candidates_cascade_add_views with the identity frame
    mapping, then the hard NMS; against merge_witness as test_cascade_passes_against_the_witness does."""
    rows, O, cap = [64, 33], 2, 128
    specs = [dict(view=None, ratios=(1.0, 1.0)), dict(view=(0.0, 0.0, 1), ratios=(1.5, 1.25))]
    S = 2 * O

    @functools.lru_cache(None)
    def gen(seed):
        import test_gpu_detect_merge as gd
        return [gd.cascade_pass(k, rows, O, 2, seed=seed, **sp) for k, sp in enumerate(specs)]

    def draw(seed):
        fw = gen(seed)
        return {f"{n}{k}{o}": fw[k][o][j] for k in range(2) for o in range(O) for j, n in enumerate(("boxes", "prob", "props"))}

    def setup(hip):
        torch = _torch()
        L = hip.lib()
        return dict(buf=torch.empty(L.mscnn_detections_candidates_bytes(S, cap), dtype=torch.uint8, device="cuda"),
                    ws=torch.empty(max(L.mscnn_detections_merge_workspace_bytes(S, cap), 1), dtype=torch.uint8, device="cuda"),
                    nbytes=L.mscnn_detections_multi_pack_bytes(S, S * cap))

    def run(hip, s, b):
        import test_gpu_detect_merge as gd
        torch = _torch()
        L = hip.lib()
        hip._check(L.mscnn_detections_candidates_reset(_vp(s["buf"]), S, cap, hip._stream()))
        for k, sp in enumerate(specs):
            outs = (hip.CascadeOutput * O)()
            for o in range(O):
                outs[o].boxes, outs[o].cls_prob, outs[o].props, outs[o].ncls = (b[f"boxes{k}{o}"].data_ptr(), b[f"prob{k}{o}"].data_ptr(),
                                                                                b[f"props{k}{o}"].data_ptr(), 2)
            descs = (hip.DetectionsDesc * S)()
            for j in range(S):
                hip._fill_desc(descs[j], 2, dict(cls_id=2, ratios=sp["ratios"], org_hw=gd.FRAME, nms_overlap=0.5))
            views = hip._view_array(None if sp["view"] is None else [sp["view"]] * 2, 2)
            R = sum(rows)
            if k == 0:
                hip._check(L.mscnn_detections_candidates_cascade_add(descs, views, C.c_float(0.1), None, k, 2, O, 1, outs, R, _vp(s["buf"]), cap,
                                                                     hip._stream()))
            else:
                hip._check(L.mscnn_detections_candidates_cascade_add_views(descs, views, (C.c_int * 2)(0, 1), C.c_float(0.1), None, k, 2, S // O, O, 1,
                                                                           outs, R, _vp(s["buf"]), cap, hip._stream()))
        pack = torch.full((s["nbytes"],), 0xFF, dtype=torch.uint8, device="cuda")
        hip._check(L.mscnn_detections_merge_fwd((C.c_double * S)(*[0.5] * S), None, S, _vp(s["buf"]), cap, _vp(pack), _vp(s["ws"]),
                                                C.c_size_t(s["ws"].numel()), hip._stream()))
        return [pack]

    def check(orc, i, o):
        import merge_witness as mw
        import test_gpu_detect_merge as gd
        import test_gpu_soft as gs
        fw = gen(SEED)
        row0 = [0, rows[0], sum(rows)]
        want = np.full(len(o[0]), 0xFF, np.uint8)
        hdr, dets, tags = gs.pack_views(want, S, cap)
        hdr[0] = [S, cap, S * cap, 0]
        for s in range(S):
            im, out = s // O, s % O
            lists = []
            for k, sp in enumerate(specs):
                boxes, prob, props = fw[k][out]
                sl = slice(row0[im], row0[im + 1])
                r, ids = mw.cascade_rows(boxes[sl], prob[sl], props[sl], 2, ratios=sp["ratios"], org_hw=gd.FRAME, det_thr=0.1)
                lists.append((mw.apply_view(r, gd.FRAME[1], sp["view"]), ids + row0[im]))
            d, pas, row, cands = mw.merge(lists)
            hdr[1 + s] = [len(d), cands, s * cap, 0]
            dets[s * cap:s * cap + len(d)] = d
            tags[s * cap:s * cap + len(d)] = (np.asarray(pas).astype(np.int32) << 24) | row
        assert hdr[1:, 0].max() > 5
        _same_bytes(o[0], want)

    case("merge_cascade_adds", ("mscnn_detections_candidates_reset", "mscnn_detections_candidates_cascade_add",
                                "mscnn_detections_candidates_cascade_add_views", "mscnn_detections_merge_fwd"), draw, run, check, setup=setup,
         workspaces=lambda s: [s["ws"]], seed=SEED)


_cascade_merge_case()


# ================================================================================================ video: tracks, render
def _tracks_case():
    """Six frames of two slots (track_cases.drift_stream): state_reset + tracks_update_fwd on one table set; the same frames as three
    frames each of two streams through tracks_update_streams_fwd, then tracks_state_reset_slots of the second stream's tables.  Ids
    and states byte for byte against the witnesses, as tests/test_gpu_track.py and _track_streams.py hold them."""
    T, K, M, SEG_CAP, N = 6, 2, 16, 24, 2
    order = [0, 1, 0, 1, 0, 1]

    @functools.lru_cache(None)
    def gen(seed):
        import track_cases as tc
        import track_streams_witness as sw
        import track_witness as tw
        frames = tc.drift_stream(seed, T=T, K=K)
        assert max(len(r) for fr in frames for r in fr if r is not None) <= SEG_CAP
        buf, offs, cap = tw.pack_bytes(frames, SEG_CAP, "merge")
        per = [tc.drift_stream(seed, T=3, K=K), tc.drift_stream(seed + 50, T=3, K=K)]
        buf2, offs2, cap2, frames2, stream_of = sw.pack_bytes(per, order, SEG_CAP, "merge")
        return dict(pack=buf, pack2=buf2), dict(frames=frames, offs=offs, cap=cap, frames2=frames2, offs2=offs2, cap2=cap2, stream_of=stream_of)

    def params():
        import track_witness as tw
        return tw.params(high_thr=0.5, low_thr=0.125, match_thr=0.1, match_thr_low=0.25, motion="linear", max_age=2, min_hits=2)

    def run(hip, s, b):
        import test_gpu_track as gt
        torch = _torch()
        L = hip.lib()
        x = gen(SEED)[1]
        p = gt.cparams(hip, params())
        state = torch.full((L.mscnn_tracks_state_bytes(K, M),), 0xFF, dtype=torch.uint8, device="cuda")
        ids = torch.full((x["cap"],), -1, dtype=torch.int32, device="cuda")
        hip._check(L.mscnn_tracks_state_reset(_vp(state), K, M, hip._stream()))
        hip._check(L.mscnn_tracks_update_fwd(C.byref(p), T, K, _vp(b["pack"]), x["cap"], _vp(state), _vp(state), M, _vp(ids), hip._stream()))
        state2 = torch.full((L.mscnn_tracks_state_bytes(N * K, M),), 0xFF, dtype=torch.uint8, device="cuda")
        ids2 = torch.full((x["cap2"],), -1, dtype=torch.int32, device="cuda")
        so = np.ascontiguousarray(x["stream_of"], dtype=np.int32)
        hip._check(L.mscnn_tracks_state_reset(_vp(state2), N * K, M, hip._stream()))
        hip._check(L.mscnn_tracks_update_streams_fwd(C.byref(p), len(x["frames2"]), K, N, so.ctypes.data_as(C.c_void_p), _vp(b["pack2"]), x["cap2"],
                                                     _vp(state2), _vp(state2), M, _vp(ids2), hip._stream()))
        before = state2.clone()
        hip._check(L.mscnn_tracks_state_reset_slots(_vp(state2), N * K, M, K, K, hip._stream()))
        return [ids, state, ids2, before, state2]

    def check(orc, i, o):
        import test_gpu_track as gt
        import track_streams_witness as sw
        import track_witness as tw
        x = gen(SEED)[1]
        p = params()
        slots = [tw.new_slot() for _ in range(K)]
        wids = tw.run(slots, x["frames"], p, M)
        _same_bytes(o[0], gt.want_ids(x["frames"], wids, x["offs"], x["cap"]))
        assert (o[0] > 0).sum() > 10, "nothing was tracked: the case shows nothing"
        _same_bytes(o[1], tw.state_bytes(slots, M, np.full(len(o[1]), 0xFF, np.uint8)))
        tables = sw.new_tables(N, K)
        wids2 = sw.run(tables, x["frames2"], x["stream_of"], p, M)
        _same_bytes(o[2], gt.want_ids(x["frames2"], wids2, x["offs2"], x["cap2"]))
        _same_bytes(o[3], sw.state_bytes(tables, M, np.full(len(o[3]), 0xFF, np.uint8)))
        tables[1] = [tw.new_slot() for _ in range(K)]                  # reset_slots: the headers of stream 1's tables, nothing else
        _same_bytes(o[4], sw.state_bytes(tables, M, o[3].copy()))

    case("tracks", ("mscnn_tracks_state_reset", "mscnn_tracks_update_fwd", "mscnn_tracks_update_streams_fwd", "mscnn_tracks_state_reset_slots"),
         lambda seed: gen(seed)[0], run, check, seed=SEED)


_tracks_case()


def _render_case():
    """Three frames of their own sizes, two slots, ids: tests/test_gpu_render.py's first case at one setting, against render_witness."""
    K = 2

    @functools.lru_cache(None)
    def gen(seed):
        import test_gpu_render as gr
        rng = np.random.default_rng(seed)
        frames = gr.frames_of(rng)
        segs = [[gr.boxes_for(rng, h, w) for _ in range(K)] for h, w in gr.SIZES]
        ids = [[gr.ids_for(rng, len(r)) for r in fr] for fr in segs]
        buf, cap, idbuf = gr.build(segs, ids, "merge")
        return dict(f0=frames[0], f1=frames[1], f2=frames[2], pack=buf, ids=idbuf), dict(frames=frames, segs=segs, ids=ids, cap=cap)

    def params():
        import render_witness as rw
        return rw.params(show_thr=0.3, thickness=3, outline_alpha=77, fill_alpha=77, label=2, label_scale=2, color_by=1, pixelate=2)

    def run(hip, s, b):
        import test_gpu_render as gr
        x = gen(SEED)[1]
        return hip.render_detections(gr.cparams(hip, params()), [b["f0"], b["f1"], b["f2"]], K, b["pack"], x["cap"], b["ids"])

    def check(orc, i, o):
        import render_witness as rw
        import test_gpu_render as gr
        x = gen(SEED)[1]
        gr.assert_frames(o, rw.render(x["frames"], x["segs"], params(), x["ids"]))
        assert all((g != f).any() for g, f in zip(o, x["frames"])), "a frame came back unchanged: the case shows nothing"

    case("render_detections", ("mscnn_render_detections_u8",), lambda seed: gen(seed)[0], run, check, seed=SEED)


_render_case()


# ================================================================================================ the census table
# C-ABI functions with a `void* stream` parameter that have NO gated case yet, each with the reason.  tests/test_stream_cases_cpu.py
# fails for a function that is neither named by a case nor listed here, and for one that is listed here but has a case.
NO_GATED_CASE = {}
