#!/usr/bin/env python3
"""Third golden file: the stock layers where a shared misreading could hide -- the pooling output shape when only one pad is
non-zero, AVE pooling over an empty window (0 / 0), ReLU on special values, one transposed convolution per family, Softmax rows
with specials, Eltwise with 8 bottoms, Concat on axis 2 -- from the REFERENCE's own layer sources (oracle/_ref).  The inputs come
from tests/stock_cases.py, so only what the reference computed is stored next to the parameters that select it.

    python tests/golden/make_golden_c.py

The archive is written with fixed member dates, so the same reference build reproduces the file byte for byte.
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(1, os.path.dirname(HERE))
import stock_cases as sc  # noqa: E402
from oracle import pyref  # noqa: E402

assert pyref.has("ref_concat"), "build oracle/_ref from this tree first: make -C oracle ref"
out = {}

# pooling on the two map sizes the device sweep uses: every combination whose shape differs from the per-dimension rule, and
# every AVE combination with a NaN in it
rows, ys, differ, nans = [], [], 0, 0
for H, W in sc.POOL_SIZES_GPU:
    x = sc.pool_input(H, W)
    for k, p, s in sc.pool_params():
        for mi, m in enumerate(("MAX", "AVE")):
            y = pyref.pool2d(x, k, p, s, m)
            d = y.shape[2:] != sc.pool_dims_per_dimension(H, W, k, p, s)
            n = bool(np.isnan(y).any())
            if d or n:
                differ += d; nans += n
                rows.append([H, W, *k, *p, *s, mi, *y.shape[2:]])
                ys.append(y.reshape(-1))
out["pool_cases"] = np.array(rows, np.int32)            # H W kh kw ph pw sh sw method Ho Wo
out["pool_y"] = np.concatenate(ys)
print(f"pooling: {len(rows)} cases ({differ} where the both-pads rule changes the shape, {nans} with NaN)")

out["relu_x"] = sc.RELU_SPECIALS
out["relu_y"] = np.stack([pyref.relu(sc.RELU_SPECIALS, slope) for slope in sc.RELU_SLOPES])

cases = sc.deconv_cases()
pick = [next(i for i, c in enumerate(cases) if c == want) for want in
        [("g1", (3, 5), (3, 2), (1, 2), True), ("g2", (5, 3), (1, 3), (0, 0), False), ("gcin", (3, 5), (1, 3), (1, 2), True),
         ("dw", (5, 3), (3, 2), (2, 1), True), ("dw", (1, 1), (3, 2), (0, 0), False)]]
out["deconv_index"] = np.array(pick, np.int32)
for i in pick:
    x, w, b, g = sc.deconv_inputs(cases[i], i)
    out[f"deconv_y{i}"] = pyref.deconv2d(x, w, b, cases[i][3], cases[i][2], g)

for tag, x in sc.softmax_inputs():
    if tag.startswith(("s0_", "s3_")) or tag in ("s2_x100", "s1_nan"):
        out[f"softmax_{tag}"] = pyref.softmax(x)

xs = sc.eltwise_inputs(8)
for op in ("PROD", "MAX", "SUM"):
    out[f"elt8_{op}"] = pyref.eltwise(xs, op)
out["elt8_coeff"] = pyref.eltwise(xs, "SUM", sc.ELTWISE_COEFFS[8])
for j, (axis, arrs) in enumerate(sc.concat_cases()):
    out[f"concat_{j}"] = pyref.concat(arrs, axis)

path = os.path.join(HERE, "reference_layers_c.npz")
with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
    for name in sorted(out):
        buf = io.BytesIO()
        np.lib.format.write_array(buf, np.ascontiguousarray(out[name]), version=(1, 0), allow_pickle=False)
        info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
        info.compress_type = zipfile.ZIP_DEFLATED
        info.external_attr = 0o644 << 16
        z.writestr(info, buf.getvalue(), compresslevel=9)
print("wrote", path, os.path.getsize(path) // 1024, "KiB,", len(out), "arrays")
