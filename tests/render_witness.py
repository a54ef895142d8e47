"""The render stage's witness: include/mscnn_hip.h's comment on mscnn_render_detections_u8 restated in numpy and plain Python loops,
rule by rule -- written from the header, not from det_render.hip.  Frames are tiny here, so every pixel walks every row.

    render(frames, segs, p, ids=None) -> the annotated copies

frames: uint8 [h, w, 3] arrays; segs[t][k]: the rows [count, 5] (x y w h score, float64) of slot k of frame t, or None for a segment
that counts as empty; ids[t][k]: that segment's track ids (int), or None.  p: params()."""
import math

import numpy as np

# 5 x 7 bitmaps, one row per byte, top row first, bit 4 = the left column: '0' .. '9', '.', ' ' (mscnn_amd/csrc/render_glyphs.h)
GLYPHS = {
    "0": (0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E),
    "1": (0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E),
    "2": (0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F),
    "3": (0x1E, 0x01, 0x01, 0x0E, 0x01, 0x01, 0x1E),
    "4": (0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02),
    "5": (0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E),
    "6": (0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E),
    "7": (0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08),
    "8": (0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E),
    "9": (0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C),
    ".": (0x00, 0x00, 0x00, 0x00, 0x00, 0x06, 0x06),
    " ": (0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00),
}
LABELS = {"none": 0, "score": 1, "id": 2, "both": 3}
COLOR_BY = {"slot": 0, "id": 1}
PALETTE = [(230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180), (70, 240, 240), (240, 50, 230)]


def params(show_thr=0.3, thickness=2, outline_alpha=256, fill_alpha=0, label=1, label_scale=1, color_by=0, pixelate=0, colors=PALETTE):
    return dict(show_thr=float(show_thr), thickness=thickness, outline_alpha=outline_alpha, fill_alpha=fill_alpha,
                label=LABELS.get(label, label), label_scale=label_scale, color_by=COLOR_BY.get(color_by, color_by), pixelate=pixelate,
                colors=[tuple(int(v) for v in c) for c in colors])


def blend(v, c, a):
    return (v * (256 - a) + c * a + 128) >> 8


def footprint(row):
    """(L, T, R, Bt) of a row, or None when it has none."""
    x, y, w, h, s = (float(v) for v in row)
    if not all(math.isfinite(v) for v in (x, y, w, h, s)):
        return None
    if max(abs(x), abs(y), abs(w), abs(h)) > 2.0 ** 30:
        return None
    L, T = math.floor(x + .5), math.floor(y + .5)
    R, Bt = math.floor((x + w) + .5) - 1, math.floor((y + h) + .5) - 1
    if R < L or Bt < T:
        return None
    return L, T, R, Bt


def label_text(score, tid, label):
    c = min(max(math.floor(float(score) * 100 + .5), 0), 100)
    sc = "1.00" if c == 100 else "0.%02d" % c
    if label == 1:
        return sc
    if label == 2:
        return str(tid) if tid > 0 else ""
    if label == 3:
        return str(tid) + " " + sc if tid > 0 else sc
    return ""


def label_rect(L, T, chars, scale, W):
    """(left, top, width, height) of a label of `chars` characters over a box whose corner is (L, T), in a frame W wide."""
    lw, lh = chars * 6 * scale, 8 * scale
    top = T - lh
    if top < 0:
        top = T
    left = L
    if left + lw > W:
        left = max(W - lw, 0)
    return left, top, lw, lh


def glyph_pixel(text, scale, dx, dy):
    """Is pixel (dx, dy) of the label rectangle of `text` a glyph pixel?"""
    ch = text[dx // (6 * scale)]
    gx, gy = (dx % (6 * scale)) // scale - 1, dy // scale - 1
    if not (0 <= gx < 5 and 0 <= gy < 7):
        return False
    return bool((GLYPHS[ch][gy] >> (4 - gx)) & 1)


def drawn_rows(segs_t, ids_t, p, H, W):
    """The drawn rows of one frame in paint order: (L, T, R, Bt, colour, text)."""
    out = []
    ncol = len(p["colors"])
    for k, rows in enumerate(segs_t):
        if rows is None:
            continue
        rows = np.asarray(rows, np.float64).reshape(-1, 5)
        for j in range(len(rows) - 1, -1, -1):
            if not rows[j, 4] >= p["show_thr"]:
                continue
            fp = footprint(rows[j])
            if fp is None:
                continue
            L, T, R, Bt = fp
            if L > W - 1 or R < 0 or T > H - 1 or Bt < 0:
                continue
            tid = int(ids_t[k][j]) if ids_t is not None and ids_t[k] is not None else 0
            col = p["colors"][tid % ncol] if p["color_by"] == 1 and tid > 0 else p["colors"][k % ncol]
            out.append((L, T, R, Bt, col, label_text(rows[j, 4], tid, p["label"])))
    return out


def render_frame(src, segs_t, ids_t, p):
    src = np.asarray(src, np.uint8)
    H, W = src.shape[:2]
    out = src.astype(np.int64)
    P, th, scale = p["pixelate"], p["thickness"], p["label_scale"]
    for L, T, R, Bt, col, text in drawn_rows(segs_t, ids_t, p, H, W):
        ink = (0, 0, 0) if 299 * col[0] + 587 * col[1] + 114 * col[2] >= 128000 else (255, 255, 255)
        for py in range(max(T, 0), min(Bt, H - 1) + 1):
            for px in range(max(L, 0), min(R, W - 1) + 1):
                if P:
                    bx0, by0 = L + (px - L) // P * P, T + (py - T) // P * P
                    blk = src[max(by0, 0):min(by0 + P - 1, Bt, H - 1) + 1, max(bx0, 0):min(bx0 + P - 1, R, W - 1) + 1].astype(np.int64)
                    n = blk.shape[0] * blk.shape[1]
                    out[py, px] = (blk.reshape(n, 3).sum(axis=0) + n // 2) // n
                if p["fill_alpha"] > 0:
                    out[py, px] = [blend(int(out[py, px, c]), col[c], p["fill_alpha"]) for c in range(3)]
                if min(px - L, R - px, py - T, Bt - py) < th:
                    out[py, px] = [blend(int(out[py, px, c]), col[c], p["outline_alpha"]) for c in range(3)]
        if text:
            left, top, lw, lh = label_rect(L, T, len(text), scale, W)
            for py in range(max(top, 0), min(top + lh, H)):
                for px in range(max(left, 0), min(left + lw, W)):
                    out[py, px] = ink if glyph_pixel(text, scale, px - left, py - top) else col
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def render(frames, segs, p, ids=None):
    return [render_frame(f, segs[t], None if ids is None else ids[t], p) for t, f in enumerate(frames)]
