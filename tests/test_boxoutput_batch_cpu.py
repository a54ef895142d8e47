"""The batched BoxOutput op without a GPU: the bindings, mscnn_boxoutput_batch_workspace_bytes (0 + an error text for a bad
descriptor, growing with num up to the 32 images of one group and not beyond, never below the per-image op's size), the host-side
refusals of mscnn_boxoutput_batch_fwd_f32 (every one comes before a device call) and Net.set_boxoutput_one_pass on a device-less net."""
import ctypes as C

import pytest

from mscnn_amd import hipapi, net as mnet, zoo

SHAPES = [(18, 60), (18, 60), (9, 30), (9, 30), (5, 15), (5, 15), (3, 8)]
FIELD = [60, 84, 120, 168, 240, 336, 480]
DS = [8, 8, 16, 16, 32, 32, 64]
FULL = [(72, 240), (72, 240), (36, 120), (36, 120), (18, 60), (18, 60), (9, 30)]      # 7s-576: 45,630 anchors


@pytest.fixture(scope="module")
def L():
    return hipapi.lib()


def desc(num=2, shapes=SHAPES, **kw):
    return hipapi.make_boxoutput_desc(shapes, num, 9, FIELD, FIELD, DS, **kw)


def test_bindings_exist(L):
    assert L.mscnn_boxoutput_batch_workspace_bytes.restype is C.c_size_t
    assert L.mscnn_boxoutput_batch_fwd_f32.argtypes == L.mscnn_boxoutput_fwd_f32.argtypes
    assert "one_pass" in hipapi.BoxOutput.__init__.__code__.co_varnames
    assert mnet.lib().mscnn_net_set_boxoutput_one_pass.argtypes == [C.c_void_p, C.c_int]


def test_workspace_bad_descriptor_is_zero_with_an_error_text(L):
    for bad in (dict(num=0), dict(num=2, nms_type="IOU", max_nms_num=-1)):
        d = desc(**bad)
        assert L.mscnn_boxoutput_batch_workspace_bytes(C.byref(d)) == 0
        assert len(L.mscnn_last_error()) > 0
    d = desc()
    d.num_heads = 0
    assert L.mscnn_boxoutput_batch_workspace_bytes(C.byref(d)) == 0 and b"heads" in L.mscnn_last_error()
    assert L.mscnn_boxoutput_batch_workspace_bytes(None) == 0 and b"null desc" in L.mscnn_last_error()


@pytest.mark.parametrize("shapes,max_nms", [(SHAPES, 2000), (SHAPES, 300), (FULL, 2000), (FULL, 4032)])
def test_workspace_grows_with_num_up_to_32_and_not_beyond(L, shapes, max_nms):
    def size(num):
        d = desc(num, shapes, max_nms_num=max_nms)
        return L.mscnn_boxoutput_batch_workspace_bytes(C.byref(d))

    d1 = desc(1, shapes, max_nms_num=max_nms)
    one = L.mscnn_boxoutput_workspace_bytes(C.byref(d1))
    assert one > 0 and size(1) >= one                            # one image is served by the per-image op on this workspace
    sizes = [size(n) for n in range(1, 33)]
    assert all(b > a for a, b in zip(sizes, sizes[1:])), sizes
    per_image = sizes[2] - sizes[1]
    assert all(b - a == per_image for a, b in zip(sizes[1:], sizes[2:]))      # one slice per image
    assert size(33) == size(32) == size(64) == size(1000)        # larger batches run as several groups on the same slices
    anchors = sum(h * w for h, w in shapes)
    k = min(max_nms, anchors, 4032)
    kb = (k + 63) // 64
    assert per_image >= anchors * (8 + 16 + 4) + kb * 64 * (16 + 4 + 4) + kb * 64 * kb * 8      # keys, boxes, scores, sorted rows, mask
    if shapes is FULL and max_nms == 2000:
        assert 32 * per_image < 70e6                             # the mask is sized by the real K bound: a group stays far below 100 MB


def test_workspace_of_the_large_path_is_the_per_image_ops(L):
    for kw in (dict(max_nms_num=0), dict(max_nms_num=6000)):
        big = [(36, 120), (36, 120), (18, 60)]
        d = hipapi.make_boxoutput_desc(big, 2, 9, FIELD[:3], FIELD[:3], DS[:3], **kw)
        assert L.mscnn_boxoutput_batch_workspace_bytes(C.byref(d)) == L.mscnn_boxoutput_workspace_bytes(C.byref(d)) > 0


def test_op_refuses_bad_arguments_before_any_device_call(L):
    fake = C.c_void_p(0x1000)                   # never dereferenced: every call below fails before a launch
    d = desc(3)
    wb = L.mscnn_boxoutput_batch_workspace_bytes(C.byref(d))
    heads = (C.c_void_p * 7)(*[0x1000] * 7)

    def call(dp=C.byref(d), heads=heads, rois=fake, props=fake, aids=fake, cap=10, count=fake, ws=fake, wbytes=wb):
        return L.mscnn_boxoutput_batch_fwd_f32(dp, heads, rois, props, aids, cap, count, ws, C.c_size_t(wbytes), None)

    def refused(text, **kw):
        rc = call(**kw)
        assert rc != 0 and text in L.mscnn_last_error(), (kw, rc, L.mscnn_last_error())
        return rc

    refused(b"null desc", dp=None)
    refused(b"null pointer", heads=None)
    refused(b"null pointer", rois=None)
    refused(b"null pointer", count=None)
    refused(b"null pointer", ws=None)
    refused(b"cap must be >= 1", cap=0)
    rc = refused(b"workspace", wbytes=wb - 1)
    d1 = desc(1)
    w1 = L.mscnn_boxoutput_workspace_bytes(C.byref(d1))
    assert rc == L.mscnn_boxoutput_fwd_f32(C.byref(d1), heads, fake, fake, fake, 10, fake, fake, C.c_size_t(w1 - 1), None)
    one_null = (C.c_void_p * 7)(*([0x1000] * 6 + [0]))
    refused(b"head 6 is null", heads=one_null)
    bad = desc(3)
    bad.channels = 5
    refused(b"channels", dp=C.byref(bad))


def test_net_switch_exists_on_a_device_less_net():
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=128, width=256, max_nms_num=60, batch=2), device=-1)
    n.set_boxoutput_one_pass(False)
    n.set_boxoutput_one_pass(True)
    n.set_boxoutput_one_pass()
