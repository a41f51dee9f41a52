"""`make sanitize-frame-diff`: tests/cpp/frame_diff_host.cpp, a stand-alone program over tsdf_amd/csrc/frame_diff_index.hpp (the frame
differences' integer arithmetic), built with the address and undefined-behaviour sanitizers on the host code and run on the CPU: the
tolerance and the states at the ends of their ranges, neighbours at row ends and corners, the clipped window, W * H = 2^32 - 1.  A
host-only check: it is skipped where hipcc is missing, and on a machine with a GPU, where sanitizer runs do not belong."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_frame_diff_arithmetic_runs_clean_under_the_host_sanitizers():
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc is missing")
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU machine: the host sanitizer run belongs on a machine without one")
    r = subprocess.run(["make", "-C", ROOT, "sanitize-frame-diff", "HIPCC=" + hipcc], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "frame_diff_host: ok" in r.stdout and "runtime error" not in r.stdout + r.stderr and "AddressSanitizer" not in r.stdout + r.stderr
