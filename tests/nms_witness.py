"""A float64 restatement of bbNms's nmsMax for the tests of the final stage's nms params: which of a list of score-sorted boxes
survive, for both types ('maxg' greedy, 'max' not) and both overlap denominators ('union', 'min').  Written from the function's
description (every box i suppresses each later box j whose overlap with it exceeds the threshold; greedy: a suppressed box suppresses
nothing), in numpy, one row of the pair matrix at a time."""
import numpy as np

TYPES = ("maxg", "max")
OVR_DNMS = ("union", "min")


def sort_rows(bbs):
    """[x y w h prob] rows in descending prob, ties in their given order (a stable sort).  Returns (rows, order)."""
    bbs = np.asarray(bbs, np.float64).reshape(-1, 5)
    order = np.argsort(-bbs[:, 4], kind="stable")
    return bbs[order], order


def overlaps(rows, ovr_dnm="union"):
    """The strict-upper-triangular overlap matrix o[i, j] (i < j) of sorted rows; -inf (over no threshold) where the boxes do not
    intersect (iw <= 0 or ih <= 0: such pairs are skipped, so a zero-area or negative-size box takes part in nothing)."""
    assert ovr_dnm in OVR_DNMS, ovr_dnm
    b = np.asarray(rows, np.float64).reshape(-1, 5)
    n = len(b)
    xs, ys = b[:, 0], b[:, 1]
    xe, ye = xs + b[:, 2], ys + b[:, 3]
    area = b[:, 2] * b[:, 3]
    out = np.full((n, n), -np.inf)
    for i in range(n - 1):
        j = np.arange(i + 1, n)
        iw = np.minimum(xe[i], xe[j]) - np.maximum(xs[i], xs[j])
        ih = np.minimum(ye[i], ye[j]) - np.maximum(ys[i], ys[j])
        hit = (iw > 0) & (ih > 0)
        o = iw * ih
        u = (area[i] + area[j]) - o if ovr_dnm == "union" else np.minimum(area[i], area[j])
        with np.errstate(divide="ignore", invalid="ignore"):
            out[i, j[hit]] = (o / u)[hit]
    return out


def nms_max(rows, overlap=0.5, greedy=True, ovr_dnm="union"):
    """Keep mask (bool[n]) of sorted [x y w h prob] rows."""
    o = overlaps(rows, ovr_dnm)
    n = len(o)
    keep = np.ones(n, bool)
    for i in range(n):
        if greedy and not keep[i]:
            continue
        keep[i + 1:] &= ~(o[i, i + 1:] > overlap)
    return keep


def keep_sets(rows, overlap=0.5):
    """{(type, ovr_dnm): keep mask} for the four combinations."""
    return {(t, d): nms_max(rows, overlap, greedy=(t == "maxg"), ovr_dnm=d) for t in TYPES for d in OVR_DNMS}
