"""Builds and runs tests/sanitize/rx_plan_check.cc, the stand-alone program over
csrc/qpsk_rx_plan.h, for tests/test_rx_plan.py (under ASan + UBSan) and for
tests/test_gpu_rx_writeset.py (a plain build: the staging limits).  Plain
module."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "singlecarrier_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def run_plan_check(tmp_dir, sanitize=True) -> str:
    """Build tests/sanitize/rx_plan_check.cc in tmp_dir, run it and return
    what it printed.  sanitize: under ASan + UBSan, as tests/test_rx_plan.py
    runs it (skipped without g++).  tests/test_gpu_rx_writeset.py reads the
    staging limits from a plain build (sanitize=False: sanitizers stay out of
    the GPU suite; a missing compiler fails there, it does not skip)."""
    if shutil.which("g++") is None:
        if sanitize:
            pytest.skip("g++ not available")
        pytest.fail("g++ not available: the staging limits come from csrc/qpsk_rx_plan.h")
    exe = str(tmp_dir / "rx_plan_check")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *(SAN if sanitize else []),
                    "-D__HIP_PLATFORM_AMD__",
                    "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    "-o", exe, os.path.join(ROOT, "tests", "sanitize", "rx_plan_check.cc")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"rx_plan_check failed ({r.returncode}):\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def plan_limits(out: str):
    """(kZeroCopyCF, the largest cf whose staging block is pinned) from the
    program's "limits" line."""
    (line,) = [l for l in out.splitlines() if l.startswith("limits ")]
    zero_copy, pinned = (int(v) for v in line.split()[1:])
    return zero_copy, pinned
