"""The routes of qpb_solve_factored_backward_multi and qpb_solve_box_backward_multi
in csrc/qpb_route.h, host only, as tests/test_route_dual_paths.py does it.

tests/route/route_multi_check.cpp (its own main, no HIP header) is built with
the host compiler under AddressSanitizer + UndefinedBehaviorSanitizer and run
directly: compiling it compiles the header's static_asserts; it holds the two
routes to the single-direction calls' classes and steps over n = 1..129 and
m = 0..257 (step 0 above n = 32 / m = 64), and walks chunks that advance the
right-hand sides and outputs by T n and T m per QP, or the right-hand sides by 0
with QPB_SHARED_RHS."""
import os
import subprocess

import pytest

from conftest import ROOT
from test_route import SAN, host_compiler

SRC = os.path.join(ROOT, "tests", "route", "route_multi_check.cpp")


def test_multi_routes():
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "route_multi_check")
        inc = ["-I", os.path.join(ROOT, "embedded-qp-solver_amd", "csrc"), "-I", os.path.join(ROOT, "include")]
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *SAN, *inc, SRC, "-o", exe],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-4000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert "runtime error:" not in out and "AddressSanitizer" not in out, out[-4000:]
    assert r.returncode == 0, out[-4000:]
    assert r.stdout.strip().endswith("route_multi_check ok")
