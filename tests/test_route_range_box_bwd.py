"""The route of qpb_solve_range_box_backward in csrc/qpb_route.h, host only, as
tests/test_route_range_box.py does it.

tests/route/route_range_box_bwd_check.cpp (its own main, no HIP header) is
built with the host compiler under AddressSanitizer + UndefinedBehaviorSanitizer
and run directly: compiling it compiles the header's static_asserts, and it
holds the route to route_bwd_dual of the materialised shape (n, mg + n), to its
two classes and to its limit over n = 1..129 and mg = 0..257."""
import os
import subprocess

import pytest

from conftest import ROOT
from test_route import SAN, host_compiler

SRC = os.path.join(ROOT, "tests", "route", "route_range_box_bwd_check.cpp")


def test_range_box_backward_route():
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "route_range_box_bwd_check")
        inc = ["-I", os.path.join(ROOT, "embedded-qp-solver_amd", "csrc"), "-I", os.path.join(ROOT, "include")]
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *SAN, *inc, SRC, "-o", exe],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-4000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert "runtime error:" not in out and "AddressSanitizer" not in out, out[-4000:]
    assert r.returncode == 0, out[-4000:]
    assert r.stdout.strip().endswith("route_range_box_bwd_check ok")
