"""The one-pass ROIAlign head without a GPU: the bindings of mscnn_roialign_ave_fwd_f32 / mscnn_roialign_ave_pair_fwd_f32 and of the
Net-level switch, every refusal of the two ops (each comes before a launch and names its argument), R == 0, and which nets
register a head at construction."""
import ctypes as C

import pytest

from mscnn_amd import hipapi, net as mnet, zoo

WIDERFACE = dict(height=160, width=192, max_nms_num=150)


@pytest.fixture(scope="module")
def L():
    return hipapi.lib()


def test_bindings_exist(L):
    vp, ci, cf = C.c_void_p, C.c_int, C.c_float
    assert L.mscnn_roialign_ave_fwd_f32.argtypes == [vp] * 3 + [ci] * 7 + [cf, cf, ci, ci, vp]
    assert L.mscnn_roialign_ave_fwd_f32.argtypes == L.mscnn_roipool_fwd_f32.argtypes
    assert L.mscnn_roialign_ave_pair_fwd_f32.argtypes == [vp] * 3 + [ci] * 7 + [cf, cf, ci, cf, ci, ci, vp]
    assert L.mscnn_roialign_ave_pair_fwd_f32.argtypes == L.mscnn_roipool_pair_fwd_f32.argtypes
    assert hipapi.roialign_ave.__code__.co_varnames[:9] == ("feat", "rois", "ph", "pw", "scale", "pad", "out", "c_total", "c_offset")
    assert hipapi.roialign_ave_pair.__code__.co_varnames[:11] == ("feat", "rois", "ph", "pw", "scale", "pad_a", "pad_b", "out", "c_total",
                                                                   "c_offset_a", "c_offset_b")
    assert mnet.lib().mscnn_net_set_roialign_one_pass.argtypes == [vp, ci]
    assert mnet.lib().mscnn_net_roialign_pairs.argtypes == [vp, vp, ci]
    assert callable(mnet.Net.set_roialign_one_pass) and callable(mnet.Net.roialign_pairs)


FAKE = 0x1000                   # never dereferenced: every call that gets it fails (or returns) before a launch


def single(L, feat=FAKE, rois=FAKE, out=FAKE, R=3, N=1, C_=8, H=9, W=12, ph=5, pw=5, c_total=8, c_offset=0):
    return L.mscnn_roialign_ave_fwd_f32(feat, rois, out, R, N, C_, H, W, ph, pw, 0.125, 0.25, c_total, c_offset, None)


def pair(L, feat=FAKE, rois=FAKE, out=FAKE, R=3, N=1, C_=8, H=9, W=12, ph=5, pw=5, off_a=0, off_b=8, c_total=16):
    return L.mscnn_roialign_ave_pair_fwd_f32(feat, rois, out, R, N, C_, H, W, ph, pw, 0.125, 0.0, off_a, 0.25, off_b, c_total, None)


@pytest.mark.parametrize("call,op", [(single, b"roialign_ave:"), (pair, b"roialign_ave_pair:")])
def test_ops_refuse_bad_arguments_before_any_launch(L, call, op):
    def refused(text, **kw):
        rc = call(L, **kw)
        err = L.mscnn_last_error()
        assert rc != 0 and err.startswith(op) and text in err, (kw, rc, err)

    refused(b"feat", feat=None)
    refused(b"rois", rois=None)
    refused(b"out", out=None)
    for name, kw in ((b"R", dict(R=-1)), (b"N", dict(N=0)), (b"C", dict(C_=0)), (b"H", dict(H=0)), (b"W", dict(W=-3)),
                     (b"pooled_h", dict(ph=0)), (b"pooled_w", dict(pw=-1))):
        refused(name + b" =", **kw)
    # the LDS table holds 256 grid points: 15 x 15 bins pass the check (R == 0: nothing is launched), 15 x 16 and 16 x 16 do not
    assert call(L, R=0, ph=15, pw=15) == 0
    assert call(L, R=0, ph=8, pw=8) == 0
    refused(b"pooled_h x pooled_w", ph=16, pw=16)
    refused(b"pooled_h x pooled_w", ph=15, pw=16)
    refused(b"pooled_h x pooled_w", ph=1, pw=200)


def test_single_op_refuses_a_window_outside_the_output(L):
    for text, kw in ((b"c_offset", dict(c_offset=-1)), (b"C_total", dict(c_total=12, c_offset=8)), (b"C_total", dict(c_total=7))):
        rc = single(L, **kw)
        assert rc != 0 and text in L.mscnn_last_error(), (kw, L.mscnn_last_error())
    assert single(L, R=0, c_total=24, c_offset=16) == 0


def test_pair_op_refuses_windows_outside_the_output_or_overlapping(L):
    def refused(text, **kw):
        rc = pair(L, **kw)
        assert rc != 0 and text in L.mscnn_last_error(), (kw, rc, L.mscnn_last_error())

    refused(b"c_offset_a", off_a=-1)
    refused(b"c_offset_b", off_b=-8)
    refused(b"c_offset_a + C", off_a=16, off_b=0, c_total=16)
    refused(b"c_offset_b + C", off_b=9, c_total=16)
    refused(b"overlap", off_a=0, off_b=7, c_total=32)
    refused(b"overlap", off_a=4, off_b=0, c_total=32)
    refused(b"overlap", off_a=3, off_b=3, c_total=32)
    assert pair(L, R=0, off_a=8, off_b=0) == 0            # windows swapped
    assert pair(L, R=0, off_a=0, off_b=16, c_total=24) == 0      # a gap between them


def test_zero_rois_return_ok_and_touch_nothing(L):
    assert single(L, R=0) == 0
    assert pair(L, R=0) == 0


def test_widerface_cascade_registers_three_heads():
    n = mnet.Net(prototxt_text=zoo.prototxt("widerface/cascade-mscnn-12s-align", **WIDERFACE), device=-1)
    heads = n.roialign_pairs()
    assert len(heads) == 3 and len(set(heads)) == 3
    aligns = [i for i, t in enumerate(n.layer_types) if t == "ROIAlign"]
    assert len(aligns) == 6
    stages = set()
    for i in heads:
        assert n.layer_types[i] == "ROIAlign"
        text = n.layer_param_text(i)
        assert "pad_ratio: 0\n" in text or "pad_ratio: 0.25\n" in text, text
        # its partner: the other ROIAlign layer on the same (split) feature and ROI blobs
        src = [b.split("_split_")[0] for b in n.layer_bottoms(i)]
        partners = [j for j in aligns if j != i and [b.split("_split_")[0] for b in n.layer_bottoms(j)] == src]
        assert len(partners) == 1 and partners[0] not in heads
        assert i < partners[0]
        stages.add(n.layer_names[i].replace("roi_grid_org", "").replace("roi_grid_ctx", ""))
        assert n.layer_kernel(i) == ""                    # nothing has been forwarded
    assert stages == {"", "_2nd", "_3rd"}
    n.set_roialign_one_pass(True)
    n.set_roialign_one_pass(False)
    n.set_roialign_one_pass()
    assert n.roialign_pairs() == heads


@pytest.mark.parametrize("model", ["kitti_car/mscnn-7s-576", "kitti_car/cascade-mscnn-7s-576-2x"])
def test_roipooling_nets_register_no_head(model):
    n = mnet.Net(prototxt_text=zoo.prototxt(model, height=128, width=256, max_nms_num=60), device=-1)
    assert n.roialign_pairs() == []
    n.set_roialign_one_pass(True)
    n.set_roialign_one_pass(False)
    n.set_roialign_one_pass()


HEAD = """
name: "head"
input: "feat" input_shape { dim: 1 dim: 8 dim: 10 dim: 12 }
input: "rois" input_shape { dim: 4 dim: 5 }
layer { name: "grid_a" type: "ROIAlign" bottom: "feat" bottom: "rois" top: "grid_a"
        roi_pooling_param { pooled_w: 5 pooled_h: 5 spatial_scale: %(scale_a)s pad_ratio: 0 } }
layer { name: "pool_a" type: "Pooling" bottom: "grid_a" top: "pool_a" pooling_param { pool: %(pool_a)s kernel_size: 2 stride: 1 } }
layer { name: "grid_b" type: "ROIAlign" bottom: "feat" bottom: "rois" top: "grid_b"
        roi_pooling_param { pooled_w: 5 pooled_h: 5 spatial_scale: 0.125 pad_ratio: 0.25 } }
layer { name: "pool_b" type: "Pooling" bottom: "grid_b" top: "pool_b" pooling_param { pool: AVE kernel_size: 2 stride: 1 } }
layer { name: "cat" type: "Concat" bottom: "%(first)s" bottom: "%(second)s" top: "cat" }
%(extra)s
"""


def head_net(**kw):
    d = dict(scale_a="0.125", pool_a="AVE", first="pool_a", second="pool_b", extra="")
    d.update(kw)
    return mnet.Net(prototxt_text=HEAD % d, device=-1)


def test_hand_written_head_is_registered_whatever_the_concat_order():
    for kw in (dict(), dict(first="pool_b", second="pool_a")):
        n = head_net(**kw)
        assert n.roialign_pairs() == [n.layer_names.index("grid_a")]


@pytest.mark.parametrize("kw", [
    dict(scale_a="0.25"),                                                                       # the two ROIAlign layers differ
    dict(extra='layer { name: "peek" type: "ReLU" bottom: "pool_a" top: "peek" }'),           # a pooled blob with a second reader
    dict(extra='layer { name: "peek" type: "ReLU" bottom: "grid_b" top: "peek" }'),           # a grid blob with a second reader
    dict(pool_a="MAX"),
], ids=["spatial_scale", "pooled_blob_read_twice", "grid_blob_read_twice", "max_pooling"])
def test_hand_written_near_heads_register_nothing(kw):
    assert head_net(**kw).roialign_pairs() == []
