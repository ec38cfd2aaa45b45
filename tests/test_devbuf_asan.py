"""CPU: the owners of device resources (csrc/devbuf.hpp: DevBuf, DevEvent, DevStream) under AddressSanitizer +
UndefinedBehaviorSanitizer with the leak check on -- growth rule, failing allocations, moves, swap, a growing vector of events, early
returns with every allocation failing in turn, the column replacement of dd_apply_migration, adopted streams.  The harness
(tools/host_asan/devbuf_harness.cpp, a program of its own) stands in for the five runtime calls and counts what is alive."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_devbuf_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "devbuf_harness"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["g++", "-g", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "gadget-2.0.7-ngravs_amd", "csrc"), "-I", os.path.join(rocm, "include"),
           os.path.join(ROOT, "tools", "host_asan", "devbuf_harness.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and ("asan" in b.stderr or "sanitize" in b.stderr):
        pytest.skip("no sanitizer runtime: " + b.stderr[-200:])
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0 and r.stdout.strip().endswith("17 cases OK"), (r.stdout[-1500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr
