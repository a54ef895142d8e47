#!/usr/bin/env python3
"""Fourth golden file: the ROI layers and DecodeBBox where a shared misreading could hide -- ROIPooling and ROIAlign at pooled sizes
on both sides of the row kernel's limit, at the smallest and the largest scale, with and without context padding, on maps with
plateaus, NaN, +-inf and signed zeros, over ROIs that leave the map on every side, are inverted, or land exactly on .5 before
roundf; DecodeBBox at every parameter set with exponents across (-104, 100), NaN / inf rows and inverted priors -- from the
REFERENCE's own layer sources (oracle/_ref).  The inputs come from tests/roi_cases.py, so only what the reference computed is
stored.

    python tests/golden/make_golden_d.py

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
import roi_cases as rc  # noqa: E402
from oracle import pyref  # noqa: E402

assert pyref.available(), "build oracle/_ref from this tree first: make -C oracle ref"
out = {}
for key, op, kind, PH, PW, scale, pad in rc.golden_d_cases():
    feat = rc.feature_map(kind, rc.std_shape(rc.SWEEP_C))
    out[key] = getattr(pyref, op)(feat, rc.golden_d_rois(scale), PH, PW, scale, pad)
print(f"roipool / roialign: {len(out)} cases")

bbox, prior = rc.decode_inputs(257)
for name, (mean, std) in rc.DECODE_PARAMS.items():
    out[f"decode_{name}"] = pyref.decode_bbox(bbox, prior, mean, std)
refused = []
for std in rc.DECODE_REFUSED_STD:
    try:
        pyref.decode_bbox(bbox, prior, (0, 0, 0, 0), std)
        refused.append(0)
    except RuntimeError:
        refused.append(1)
out["decode_refused"] = np.array(refused, np.int32)          # 1: the reference's set-up refused this std
print("decode: refused", refused)

path = os.path.join(HERE, "reference_layers_d.npz")
with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
    for name in sorted(out):
        buf = io.BytesIO()
        np.lib.format.write_array(buf, np.ascontiguousarray(out[name]), version=(1, 0), allow_pickle=False)
        info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
        info.compress_type = zipfile.ZIP_DEFLATED
        info.external_attr = 0o644 << 16
        z.writestr(info, buf.getvalue(), compresslevel=9)
print("wrote", path, os.path.getsize(path) // 1024, "KiB,", len(out), "arrays")
