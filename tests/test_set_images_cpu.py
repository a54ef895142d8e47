"""The batched pre-processing op without a GPU: mscnn_preprocess_batch_workspace_bytes (every frame's intermediate at a 256-byte aligned
offset, back to back) and the host-side argument checks of mscnn_preprocess_batch_u8_f32 (every refusal comes before a launch)."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    L = C.CDLL(os.path.join(ROOT, "mscnn_amd/libmscnn_hip.so"))
    L.mscnn_last_error.restype = C.c_char_p
    L.mscnn_preprocess_workspace_bytes.restype = C.c_size_t
    L.mscnn_preprocess_batch_workspace_bytes.restype = C.c_size_t
    L.mscnn_preprocess_batch_workspace_bytes.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.mscnn_preprocess_batch_u8_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                                C.c_void_p, C.c_size_t, C.c_void_p]
    return L


def ints(v):
    return (C.c_int * max(len(v), 1))(*v)


def align(b):
    return (b + 255) // 256 * 256


# (org_h, org_w) against a 576 x 1920 target: KITTI frames (grow on both axes), one that shrinks on both, one that shrinks on H and
# grows on W, one that grows on H and shrinks on W, one at the target size, odd sizes whose intermediates are not multiples of 256
ORGS = [(375, 1242), (370, 1224), (1200, 4000), (900, 1000), (300, 2500), (576, 1920), (7, 3), (1, 1)]


def test_workspace_is_the_aligned_sum_of_the_per_frame_sizes(L):
    H, W = 576, 1920
    per = [L.mscnn_preprocess_workspace_bytes(h, w, H, W) for h, w in ORGS]
    assert per[2] == 1200 * W * 3 and per[3] == H * 1000 * 3          # the smaller scale goes first: W-first, then H-first
    assert any(p % 256 for p in per)
    for n in range(1, len(ORGS) + 1):
        hs, ws = [o[0] for o in ORGS[:n]], [o[1] for o in ORGS[:n]]
        got = L.mscnn_preprocess_batch_workspace_bytes(n, ints(hs), ints(ws), H, W)
        assert got == sum(align(p) for p in per[:n]) and got >= sum(per[:n]), n
    assert L.mscnn_preprocess_batch_workspace_bytes(1, ints([375]), ints([1242]), 57, 191) == align(
        L.mscnn_preprocess_workspace_bytes(375, 1242, 57, 191))
    # refused arguments size nothing
    assert L.mscnn_preprocess_batch_workspace_bytes(0, ints([375]), ints([1242]), H, W) == 0
    assert L.mscnn_preprocess_batch_workspace_bytes(2, ints([375, 0]), ints([1242, 1224]), H, W) == 0
    assert L.mscnn_preprocess_batch_workspace_bytes(1, ints([375]), ints([1242]), H, 0) == 0
    assert L.mscnn_preprocess_batch_workspace_bytes(1, None, ints([1242]), H, W) == 0


def test_op_refuses_bad_arguments_before_any_launch(L):
    fake = C.c_void_p(0x1000)                  # never dereferenced: every call below fails before a launch
    mean = (C.c_float * 3)(104, 117, 123)
    H, W = 64, 96

    def call(count=2, hs=(375, 370), ws=(1242, 1224), imgs="ok", out=fake, H=H, W=W, mean=mean, work=fake, wbytes=None, orgs=True):
        n = max(len(hs), 1)
        ptrs = (C.c_void_p * n)(*([0x2000] * n)) if imgs == "ok" else imgs
        h, w = (ints(hs), ints(ws)) if orgs else (None, None)
        if wbytes is None:
            wbytes = 1 << 40
        rc = L.mscnn_preprocess_batch_u8_f32(ptrs, h, w, count, out, H, W, mean, work, C.c_size_t(wbytes), None)
        return rc, L.mscnn_last_error().decode()

    cases = [
        (dict(imgs=None), "null pointer"),
        (dict(orgs=False), "null pointer"),
        (dict(out=None), "null pointer"),
        (dict(mean=None), "null pointer"),
        (dict(work=None), "null pointer"),
        (dict(imgs=(C.c_void_p * 2)(0x2000, None)), "image 1 is a null pointer"),
        (dict(count=0), "count 0 < 1"),
        (dict(count=-3), "count -3 < 1"),
        (dict(H=0), "bad output shape 0 x 96"),
        (dict(W=-1), "bad output shape 64 x -1"),
        (dict(hs=(375, 0)), "image 1 has bad shape 0 x 1224"),
        (dict(ws=(-5, 1224)), "image 0 has bad shape 375 x -5"),
    ]
    for kw, msg in cases:
        rc, err = call(**kw)
        assert rc != 0 and msg in err, (kw, rc, err)
    need = L.mscnn_preprocess_batch_workspace_bytes(2, ints([375, 370]), ints([1242, 1224]), H, W)
    rc, err = call(wbytes=need - 1)
    assert rc != 0 and f"workspace {need - 1} bytes < {need}" in err, err
    # the aligned sum is needed, not the plain sum
    plain = sum(L.mscnn_preprocess_workspace_bytes(h, w, H, W) for h, w in [(375, 1242), (370, 1224)])
    assert plain < need
    rc, err = call(wbytes=plain)
    assert rc != 0 and "workspace" in err, err


def test_net_set_images_refuses_before_touching_the_device():
    """mscnn_net_set_images' preconditions on a graph-only net (device -1: no HIP device is touched): count == num(), sizes > 0; and
    Net.set_images' own checks of the frames."""
    import numpy as np
    from mscnn_amd import net as mnet, zoo
    n = mnet.Net(prototxt_text=zoo.prototxt("kitti_car/mscnn-7s-576", height=192, width=640, batch=4), device=-1)
    f = np.zeros((10, 20, 3), np.uint8)
    cases = [([f] * 3, "3 images for blob data of shape 4 3 192 640"),
             ([f] * 5, "5 images for blob data"),
             ([], "0 images for blob data"),
             ([f] * 3 + [np.zeros((0, 20, 3), np.uint8)], "image 3 is 0 x 20"),
             ([f] * 3 + [f.astype(np.float32)], "frame 3 is not a uint8"),
             ([f] * 3 + [f[:, :, :2]], "frame 3 is not a uint8"),
             ([f] * 3 + [f[:, :, 0]], "frame 3 is not a uint8")]
    for frames, msg in cases:
        with pytest.raises(mnet.NetError, match=msg):
            n.set_images("data", frames)
    with pytest.raises(mnet.NetError, match="Unknown blob name"):
        n.set_images("nope", [f] * 4)
