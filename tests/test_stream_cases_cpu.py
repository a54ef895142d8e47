"""Census of the stream contract's cases: every function of include/mscnn_hip.h with a `void* stream` parameter is named by a
gated case of tests/stream_cases.py (each case declares the ABI functions it runs), or stands in its NO_GATED_CASE table with a
written reason.  A new entry point with a stream fails this test until it has a case."""
import os
import re

from tests import stream_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def abi_functions_with_a_stream():
    text = open(os.path.join(ROOT, "include", "mscnn_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = []
    for m in re.finditer(r"MSCNN_API\s+[\w\s\*]+?\b(mscnn_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S):
        if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2)):
            out.append(m.group(1))
    return out


def test_the_parser_sees_the_header():
    fns = abi_functions_with_a_stream()
    assert len(fns) == len(set(fns)) >= 60, len(fns)
    for known in ("mscnn_conv2d_fwd_f32", "mscnn_inner_product_fwd_f16", "mscnn_store_words_i32", "mscnn_tracks_update_streams_fwd",
                  "mscnn_preprocess_views_u8_f32", "mscnn_render_detections_u8"):
        assert known in fns
    assert "mscnn_conv2d_plan_create" not in fns and "mscnn_wgemm_force_whole_tiles" not in fns


def test_every_stream_function_has_a_gated_case():
    fns = set(abi_functions_with_a_stream())
    named = {f for c in stream_cases.CASES for f in c.abi}
    assert named <= fns, f"cases name functions the header does not declare with a stream: {sorted(named - fns)}"
    listed = set(stream_cases.NO_GATED_CASE)
    assert listed <= fns, sorted(listed - fns)
    assert not (listed & named), f"listed as uncovered but named by a case: {sorted(listed & named)}"
    for f, reason in stream_cases.NO_GATED_CASE.items():
        assert isinstance(reason, str) and len(reason.split()) >= 5, f"{f}: the table wants a written reason"
    missing = sorted(fns - named - listed)
    assert not missing, f"no gated case names {missing}"


def test_case_names_are_unique_and_cases_declare_their_abi():
    names = [c.name for c in stream_cases.CASES]
    assert len(names) == len(set(names))
    for c in stream_cases.CASES:
        assert c.abi, c.name
        assert c.busy or c.why, c.name
