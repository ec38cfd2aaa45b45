"""CPU: the host row loops of the column layer (csrc/rows.hpp: gather, scatter, masked scatter) under AddressSanitizer +
UndefinedBehaviorSanitizer -- n in {0, 1, 2, 257}, rows of 1, 4, 8 and 24 bytes, stride == row and stride > row, on buffers that end
with the last row's field, each against a byte-wise restatement (tools/host_asan/rows_harness.cpp, a program of its own)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_loops_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "rows_harness"
    cmd = ["g++", "-g", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I", os.path.join(ROOT, "gadget-2.0.7-ngravs_amd", "csrc"), os.path.join(ROOT, "tools", "host_asan", "rows_harness.cpp"),
           "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and ("asan" in b.stderr or "sanitize" in b.stderr):
        pytest.skip("no sanitizer runtime: " + b.stderr[-200:])
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0 and r.stdout.strip().endswith("48 cases OK"), (r.stdout[-1500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr
