"""The slice plan of qpb_solve_shared_backward's batch sum (qpb::sum_plan in
csrc/qpb_route.h), host only.

tests/shared/plan_check.cpp (its own main, no HIP header) is built with the
host compiler under AddressSanitizer + UndefinedBehaviorSanitizer and run
directly, as tests/test_route.py does: over batches 1 .. 5000 and a few up to
2^40 every QP lies in exactly one slice, slice starts are multiples of 4 and
the slot count stays under its cap.  qpb.sum_plan, the Python mirror the GPU
tests choose their batches with, must give the same plan."""
import os
import subprocess

import pytest

from conftest import ROOT
from test_route import SAN, host_compiler

SRC = os.path.join(ROOT, "tests", "shared", "plan_check.cpp")
BATCHES = [1, 4, 5, 67, 127, 128, 129, 293, 5000, 131072, 131073, 1 << 20, (1 << 20) + 1, 1 << 40]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("plan") / "plan_check")
    inc = ["-I", os.path.join(ROOT, "embedded-qp-solver_amd", "csrc"), "-I", os.path.join(ROOT, "include")]
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *SAN, *inc, SRC, "-o", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert "runtime error:" not in out and "AddressSanitizer" not in out, out[-4000:]
    assert r.returncode == 0, out[-4000:]
    return r.stdout


def test_slices_tile_every_batch(exe):
    assert _run(exe).strip().endswith("plan_check ok")


def test_python_mirror_gives_the_same_plan(exe):
    if os.environ.get("QPB_SANITIZED"):
        return  # imports the library
    import qpb
    lines = _run(exe, *[str(b) for b in BATCHES]).split("\n")
    for b, line in zip(BATCHES, lines):
        assert tuple(int(v) for v in line.split()) == qpb.sum_plan(b), b
    assert qpb.sum_plan(0) == (0, 0)
