"""The native driver's host-only units under sanitizers: csrc/tests/driver_selftest.cpp, a stand-alone program with
its own main (the bounded frame read-ahead of --batch_frames on a synthetic source, the --profile JSON-line builder),
built with g++ and run the way tests/test_fit_sanitizers.py builds and runs the fit diagnostics': once under
AddressSanitizer + UndefinedBehaviorSanitizer, once under ThreadSanitizer (skipped where its runtime is not installed:
the link fails)."""
import os
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "csrc" / "tests" / "driver_selftest.cpp"


def _build_and_run(tmp_path, name, sanitize, env, skip_without_runtime=False):
    exe = tmp_path / name
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", *sanitize, "-pthread", str(SRC), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and skip_without_runtime and ("-ltsan" in r.stderr or "libtsan" in r.stderr):
        pytest.skip("the thread sanitizer's runtime is not installed: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "driver selftest OK" in r.stdout


def test_driver_host_units_asan_ubsan(tmp_path):
    _build_and_run(tmp_path, "driver_selftest_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
                   dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
                        UBSAN_OPTIONS="print_stacktrace=1"))


def test_driver_host_units_tsan(tmp_path):
    _build_and_run(tmp_path, "driver_selftest_tsan", ["-fsanitize=thread"],
                   dict(TSAN_OPTIONS="halt_on_error=1:second_deadlock_stack=1"), skip_without_runtime=True)
