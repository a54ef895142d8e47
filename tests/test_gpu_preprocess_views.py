"""Pre-processing of views on the GPU: mscnn_preprocess_views_u8_f32 against its definition -- every slice bit-identical to
mscnn_preprocess_u8_f32 on a contiguous host copy of the window (mirrored with [:, ::-1] when flip_x) and to the numpy witness
(tests/views_witness.py: crop / mirror, then oracle.pyoracle.preprocess).  Two frames of 37 x 53 and 41 x 29, output 24 x 40; no
tolerance is involved anywhere."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import guarded                                   # noqa: E402
import views_witness as vw                       # noqa: E402

H, W = 24, 40
ORGS = [(37, 53), (41, 29)]


def V(frame, x0, y0, w, h, flip_x=0):
    return dict(frame=frame, x0=x0, y0=y0, w=w, h=h, flip_x=flip_x)


# name -> (view, the pass that runs first: "H" when H / h <= W / w)
VIEWS = {
    "whole frame 0 (both axes reduced)": (V(0, 0, 0, 53, 37), "H"),
    "odd offset (both axes enlarged)": (V(0, 5, 3, 31, 20), "H"),
    "its mirror": (V(0, 5, 3, 31, 20, 1), "H"),
    "enlarged in both axes, W first": (V(1, 2, 4, 20, 6), "W"),
    "reduced in both axes, W first": (V(0, 1, 2, 50, 25), "W"),
    "reduced in both axes, mirrored": (V(0, 1, 2, 50, 33, 1), "H"),
    "whole frame 1: H shrinks, W grows": (V(1, 0, 0, 29, 41), "H"),
    "H grows, W shrinks": (V(0, 0, 10, 53, 12), "W"),
    "H grows, W shrinks, mirrored": (V(0, 0, 10, 53, 12, 1), "W"),
    "one pixel wide": (V(0, 7, 0, 1, 37), "H"),
    "one pixel wide and high, mirrored": (V(1, 28, 40, 1, 1, 1), "H"),
    "touching the last row and column of frame 0": (V(0, 49, 32, 4, 5), "H"),
    "touching the last row and column of frame 1": (V(1, 20, 30, 9, 11, 1), "H"),
}
# (the table's own claims: which pass runs first, and that both orders occur among enlarged, reduced and mixed windows)
for _name, (_v, _first) in VIEWS.items():
    assert ("H" if H / _v["h"] <= W / _v["w"] else "W") == _first, _name
assert {f for _, f in VIEWS.values()} == {"H", "W"}


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X: torch.cuda.is_available() is False")
    from mscnn_amd import hipapi
    hipapi.lib()
    return hipapi


def rgb(h, w, seed):
    """uint8 RGB [h, w, 3], pixels <= 200 (a guard band of 255 never looks like a pixel): blocky noise with fine noise on top."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0, 200, (h // 5 + 1, w // 5 + 1, 3))
    img = np.repeat(np.repeat(base, 5, 0), 5, 1)[:h, :w] + rng.normal(0, 8, (h, w, 3))
    return np.ascontiguousarray(np.clip(img, 0, 200).astype(np.uint8))


@pytest.fixture(scope="module")
def frames():
    return [rgb(h, w, 71 + i) for i, (h, w) in enumerate(ORGS)]


@pytest.fixture(scope="module")
def reference(frames, orc):
    """The witness's slices of every view of VIEWS, computed once; left unchanged."""
    ref = vw.preprocess_views(orc, frames, [v for v, _ in VIEWS.values()], H, W)
    ref.setflags(write=False)
    return ref


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_every_slice_is_the_single_frame_op_on_the_host_crop_and_the_witness(hip, frames, reference):
    views = [v for v, _ in VIEWS.values()]
    out = hip.preprocess_views([dev(f) for f in frames], views, H, W).cpu().numpy()
    assert out.shape == (len(views), 3, H, W) and out.dtype == np.float32 and np.isfinite(reference).all()
    for i, (name, (v, _)) in enumerate(VIEWS.items()):
        one = hip.preprocess(dev(vw.crop(frames[v["frame"]], v)), H, W).cpu().numpy()
        assert np.array_equal(out[i:i + 1], one), name
        assert np.array_equal(out[i], reference[i]), name
    # the mirror of a window is another image to the resize: the two slices differ on these frames
    assert not np.array_equal(out[1], out[2])


def test_no_pixel_outside_the_windows_is_read(hip, frames, reference):
    keep = [i for i, (v, _) in enumerate(VIEWS.values()) if (v["h"], v["w"]) != ORGS[v["frame"]]]
    views = [list(VIEWS.values())[i][0] for i in keep]
    other = []
    for f, fr in enumerate(frames):
        m = vw.outside_mask(fr.shape[:2], views, frame=f)
        assert m.sum() > fr.shape[0] * fr.shape[1] // 10, "the windows leave too little of the frame to show anything"
        g = fr.copy()
        g[m] = 200 - g[m]
        assert not np.array_equal(g, fr)
        other.append(g)
    out = hip.preprocess_views([dev(g) for g in other], views, H, W).cpu().numpy()
    assert np.array_equal(out, reference[keep])


def test_33_views_cross_the_launch_table_and_a_custom_mean(hip, frames, reference, orc):
    views = [v for v, _ in VIEWS.values()]
    many = (views * 3)[:33]
    assert many[32] is views[32 % len(views)] and len(views) == 13
    out = hip.preprocess_views([dev(f) for f in frames], many, H, W).cpu().numpy()
    for i in range(33):
        assert np.array_equal(out[i], reference[i % len(views)]), i
    many = [views[0]] + views[1:] * 3
    many = many[:32] + [views[0]]
    out = hip.preprocess_views([dev(f) for f in frames], many, H, W, mean_bgr=(1.5, 2.25, 100.0)).cpu().numpy()
    assert np.array_equal(out[32], out[0]), "slice 32 (the second launch) is the view of slice 0"
    assert np.array_equal(out[0:1], orc.preprocess(frames[0], H, W, mean_bgr=(1.5, 2.25, 100.0)))


def test_buffer_contract_guards_and_an_unaligned_workspace(hip, frames, reference, monkeypatch):
    """out and the workspace between guard bands, the frames as guarded inputs (guards of 255: no pixel is): the guards are intact,
    the frames unwritten, every byte of out written; a workspace base that is not 16-byte aligned is refused before any launch."""
    arena = guarded.Arena("cuda")
    monkeypatch.setattr(hip, "torch", guarded.GuardedTorch(torch, arena))
    views = [v for v, _ in VIEWS.values()]
    fr = [arena.input(f, 255) for f in frames]
    out = hip.preprocess_views(fr, views, H, W)
    torch.cuda.synchronize()
    arena.check()
    assert not arena.record(out).is_input and np.array_equal(out.cpu().numpy(), reference)
    # the workspace is exactly as large as the _bytes function says: one byte less is refused
    va = hip.view_array(views)
    need = hip.lib().mscnn_preprocess_views_workspace_bytes(va, len(views), H, W)
    assert need > 0 and need % 256 == 0
    ws = arena.alloc(need + 16, torch.uint8)
    out2 = arena.alloc((len(views), 3, H, W), torch.float32)
    with pytest.raises(hip.MscnnError, match="workspace must be 16-byte aligned"):
        hip.preprocess_views(fr, views, H, W, out=out2, ws=ws[8:8 + need])
    with pytest.raises(hip.MscnnError, match=f"workspace {need - 1} bytes < {need}"):
        hip.preprocess_views(fr, views, H, W, out=out2, ws=ws[:need - 1])
    torch.cuda.synchronize()
    assert guarded.all_poison(out2) and guarded.all_poison(ws)
    hip.preprocess_views(fr, views, H, W, out=out2, ws=ws[:need])
    torch.cuda.synchronize()
    arena.check()
    assert np.array_equal(out2.cpu().numpy(), reference) and guarded.all_poison(ws[need:])
