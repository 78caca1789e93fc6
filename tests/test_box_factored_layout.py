"""The box factor buffer's layout (csrc/qpb_factor.h, bxfct) and
route_box_factored (csrc/qpb_route.h), host only.

tests/box_factored/layout_check.cpp (its own main, no HIP header) is built with
the host compiler under AddressSanitizer + UndefinedBehaviorSanitizer and run
directly, as tests/test_route.py builds its program: the two headers'
static_asserts compile, and the program checks the sections, their alignment and
the class boundary against the route at every n up to past the limit."""
import os
import subprocess

import pytest

from conftest import ROOT
from test_route import SAN, host_compiler

SRC = os.path.join(ROOT, "tests", "box_factored", "layout_check.cpp")


def test_layout_and_route(tmp_path):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "layout_check")
    inc = ["-I", os.path.join(ROOT, "embedded-qp-solver_amd", "csrc"), "-I", os.path.join(ROOT, "include")]
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *SAN, *inc, SRC, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert "runtime error:" not in out and "AddressSanitizer" not in out, out[-4000:]
    assert r.returncode == 0, out[-4000:]
    assert r.stdout.strip().endswith("layout_check ok")
