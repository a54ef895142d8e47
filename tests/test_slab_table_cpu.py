"""The stream table of the InnerProduct slab buffers (mscnn_amd/csrc/slab_table.h, used by reserve_slabs in gemm.hip) on the host:
tests/slab_table_main.cpp is compiled with AddressSanitizer and UBSan into a stand-alone program and run.  It drives the table with
one stream, with as many streams as slots, and with more streams than slots (least-recently-used eviction), handling malloc'ed
stand-in buffers the way reserve_slabs handles device buffers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slab_table_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ / clang++ / c++) to build tests/slab_table_main.cpp")
    exe = tmp_path / "slab_table_main"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "mscnn_amd", "csrc"), os.path.join(ROOT, "tests", "slab_table_main.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "slab table ok" in r.stdout, r.stdout + r.stderr
