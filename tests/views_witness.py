"""A numpy restatement of the views of a frame run as one batch (mscnn_preprocess_views_u8_f32, mscnn_detections_candidates_add_views,
Net.set_image_views / detect_merge_add(..., list_of=)).  No pin on the reference -- its scripts have neither views nor a merge -- so
this is the check.

  * pre-processing: a view is a numpy crop of its frame, mirrored with [:, ::-1] when flip_x, made contiguous and handed to
    oracle.pyoracle.preprocess: the resize sees the window alone (its borders, its size, its pass order);
  * candidates: the images of a batched forward are the passes of tests/merge_witness.py, listed per list in (add call, image index
    ascending) order; the tag's pass is the ADD CALL, its row is absolute in the batch.

TEST INFRASTRUCTURE ONLY."""
import numpy as np

import merge_witness as mw


def crop(frame, view):
    """The window of a view as a contiguous uint8 [h, w, 3] array.  view: dict x0, y0, w, h, flip_x (0)."""
    x0, y0, w, h = (int(view[k]) for k in ("x0", "y0", "w", "h"))
    H, W = frame.shape[:2]
    if not (w >= 1 and h >= 1 and 0 <= x0 and 0 <= y0 and x0 + w <= W and y0 + h <= H):
        raise ValueError(f"window {h} x {w} at ({x0}, {y0}) is not inside a {H} x {W} frame")
    win = frame[y0:y0 + h, x0:x0 + w]
    if view.get("flip_x", 0):
        win = win[:, ::-1]
    return win.copy(order="C")      # (a copy, never a view: a mirrored 1-pixel window would keep its negative stride)


def preprocess_views(orc, frames, views, H, W, mean_bgr=(104.0, 117.0, 123.0)):
    """[len(views), 3, H, W] float32: slice v = the oracle's preprocess of view v's window."""
    return np.concatenate([orc.preprocess(crop(frames[v.get("frame", 0)], v), H, W, mean_bgr=mean_bgr) for v in views])


def outside_mask(frame_hw, views, frame=0):
    """bool [h, w]: the pixels of frame `frame` that no view's window holds."""
    m = np.ones(frame_hw, bool)
    for v in views:
        if v.get("frame", 0) == frame:
            m[v["y0"]:v["y0"] + v["h"], v["x0"]:v["x0"] + v["w"]] = False
    return m


def list_passes(adds, list_of_per_add, frame):
    """adds: per add call, per image of its batch, (rows [n, 5] in frame coordinates, row ids [n]) for ONE slot; list_of_per_add: per
    add call the frame of each image.  -> ([(rows, ids)] in (add, image) order for the lists of `frame`, the add call of each)."""
    passes, add_of = [], []
    for a, (images, list_of) in enumerate(zip(adds, list_of_per_add)):
        for b, item in enumerate(images):
            if list_of[b] == frame:
                passes.append(item)
                add_of.append(a)
    return passes, add_of


def merge_views(adds, list_of_per_add, frame, overlap=0.5, type="maxg", ovr_dnm="union"):
    """merge_witness.merge over the images that go to `frame`'s list, in (add, image) order.  Returns (dets, pass = ADD CALL of each
    detection, row, candidates, image-level pass index as merge_witness counts it)."""
    passes, add_of = list_passes(adds, list_of_per_add, frame)
    if not passes:
        return np.zeros((0, 5)), np.zeros(0, np.int32), np.zeros(0, np.int32), 0, np.zeros(0, np.int32)
    dets, pas, row, cands = mw.merge(passes, overlap, type, ovr_dnm)
    return dets, np.asarray(add_of, np.int32)[pas], row, cands, pas


def candidate_list(adds, list_of_per_add, frame):
    """The list itself before the NMS: (rows [n, 5], tags [n]) in (add, image, row) order, tag = (add << 24) | row."""
    passes, add_of = list_passes(adds, list_of_per_add, frame)
    rows = np.concatenate([np.asarray(r, np.float64).reshape(-1, 5) for r, _ in passes]) if passes else np.zeros((0, 5))
    tags = np.concatenate([(a << 24) | np.asarray(i, np.int32) for a, (_, i) in zip(add_of, passes)]) if passes else np.zeros(0, np.int32)
    return rows, tags.astype(np.int32)


def self_check():
    """The witness's own checks (run by tests/test_views_cpu.py)."""
    f = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    w = crop(f, dict(x0=2, y0=1, w=3, h=2))
    assert w.flags["C_CONTIGUOUS"] and np.array_equal(w, f[1:3, 2:5])
    m = crop(f, dict(x0=2, y0=1, w=3, h=2, flip_x=1))
    assert m.flags["C_CONTIGUOUS"] and np.array_equal(m, f[1:3, 4:1:-1]) and np.array_equal(m[:, ::-1], w)
    assert np.array_equal(crop(f, dict(x0=0, y0=0, w=7, h=5)), f)
    for bad in (dict(x0=5, y0=0, w=3, h=2), dict(x0=0, y0=4, w=1, h=2), dict(x0=-1, y0=0, w=2, h=2), dict(x0=0, y0=0, w=0, h=2)):
        try:
            crop(f, bad)
        except ValueError:
            continue
        raise AssertionError(bad)
    o = outside_mask((5, 7), [dict(x0=2, y0=1, w=3, h=2), dict(x0=0, y0=0, w=1, h=5, frame=1)])
    assert o.sum() == 35 - 6 and not o[1:3, 2:5].any()
    # two adds of (2 images, 1 image); images 0 and 2 (of add 0: 0 and 1 -> frames 0, 1; add 1: image 0 -> frame 0)
    a = (np.array([[0.0, 0.0, 10.0, 10.0, 0.9]]), np.array([3], np.int32))
    b = (np.array([[100.0, 0.0, 10.0, 10.0, 0.8]]), np.array([7], np.int32))
    c = (np.array([[1.0, 0.0, 10.0, 10.0, 0.95]]), np.array([0], np.int32))
    adds, lof = [[a, b], [c]], [[0, 1], [0]]
    rows, tags = candidate_list(adds, lof, 0)
    assert rows[:, 4].tolist() == [0.9, 0.95] and tags.tolist() == [3, (1 << 24) | 0]
    dets, pas, row, cands, _ = merge_views(adds, lof, 0)
    assert dets[:, 4].tolist() == [0.95] and pas.tolist() == [1] and row.tolist() == [0] and cands == 2
    dets, pas, row, cands, _ = merge_views(adds, lof, 1)
    assert dets[:, 4].tolist() == [0.8] and pas.tolist() == [0] and row.tolist() == [7] and cands == 1
    assert merge_views(adds, lof, 2)[3] == 0
