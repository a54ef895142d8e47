"""A restatement of the window rule of mscnn_net_crops (include/mscnn_net.h: steps 1 - 7, order and bound) in plain Python floats and
ints, written from that comment.  Python's float is the C double and every operator rounds once, so the doubles of steps 2 - 4 are the
header's; from the four floors on the numbers are Python ints.  The pixels are not restated: a patch is the single-frame op on a host
copy of its window (tests/views_witness.py restates that op).

  params(...)                       the keywords of mscnn_amd.net.crops_params as a dict, ints for fit / border
  window(p, row, org_h, org_w)      (x0, y0, w, h) or None
  crops(frames, segs, p, ids)       frames: [(org_h, org_w)] or arrays with .shape; segs[b][k] = rows [D, 5]; ids[b][k] = int ids or None
                                    -> ([(frame, slot, row, track_id, x0, y0, w, h)], dropped)"""
import math

BORDERS = {"clip": 0, "shift": 1}
LIMIT = 2.0 ** 30


def params(size=(128, 64), thr=0.3, context=1.0, fit=False, border="clip", min_size=1, max_crops=1, slot=None, tracked_only=False,
           mean=(0, 0, 0)):
    return dict(out_h=int(size[0]), out_w=int(size[1]), thr=float(thr), context=float(context), fit=int(fit), border=int(BORDERS.get(border, border)),
                min_size=int(min_size), max_crops=int(max_crops), slot=-1 if slot is None else int(slot), tracked_only=int(tracked_only),
                mean=tuple(float(v) for v in mean))


def window(p, row, org_h, org_w):
    x, y, w, h, s = (float(v) for v in row)
    # 1
    if not s >= p["thr"]:
        return None
    if not all(math.isfinite(v) for v in (x, y, w, h, s)):
        return None
    if not w > 0 or not h > 0:
        return None
    if abs(x) > LIMIT or abs(y) > LIMIT or w > LIMIT or h > LIMIT:
        return None
    # 2
    ww = w * p["context"]
    hh = h * p["context"]
    # 3
    if p["fit"] == 1:
        a = float(p["out_w"]) / float(p["out_h"])
        t = hh * a
        if ww < t:
            ww = t
        else:
            hh = ww / a
    # 4
    cx = x + w / 2
    cy = y + h / 2
    x0 = cx - ww / 2
    y0 = cy - hh / 2
    L = math.floor(x0 + .5)
    T = math.floor(y0 + .5)
    R = math.floor((x0 + ww) + .5) - 1
    B = math.floor((y0 + hh) + .5) - 1
    Wd = R - L + 1
    Ht = B - T + 1
    if Wd < 1 or Ht < 1:
        return None
    if p["border"] == 1:
        # 5
        if Wd >= org_w:
            L, Wd = 0, org_w
        elif L < 0:
            L = 0
        elif L + Wd > org_w:
            L = org_w - Wd
        if Ht >= org_h:
            T, Ht = 0, org_h
        elif T < 0:
            T = 0
        elif T + Ht > org_h:
            T = org_h - Ht
    else:
        # 6
        L1, R1 = max(L, 0), min(R, org_w - 1)
        T1, B1 = max(T, 0), min(B, org_h - 1)
        if L1 > R1 or T1 > B1:
            return None
        L, T, Wd, Ht = L1, T1, R1 - L1 + 1, B1 - T1 + 1
    # 7
    if Wd < p["min_size"] or Ht < p["min_size"]:
        return None
    return (L, T, Wd, Ht)


def crops(frames, segs, p, ids=None):
    out, dropped = [], 0
    for b, fr in enumerate(segs):
        org_h, org_w = (frames[b].shape if hasattr(frames[b], "shape") else frames[b])[:2]
        for k, rows in enumerate(fr):
            if p["slot"] >= 0 and k != p["slot"]:
                continue
            for j, row in enumerate(rows if rows is not None else []):
                tid = int(ids[b][k][j]) if ids is not None and ids[b][k] is not None else 0
                if p["tracked_only"] and not tid > 0:
                    continue
                win = window(p, row, int(org_h), int(org_w))
                if win is None:
                    continue
                if len(out) >= p["max_crops"]:
                    dropped += 1
                    continue
                out.append((b, k, j, tid) + win)
    return out, dropped
