"""The route table and the chunk walker of csrc/qpb_route.h, host only.

tests/route/route_check.cpp (its own main, no HIP header) is built with the
host compiler under AddressSanitizer + UndefinedBehaviorSanitizer and run
directly: it compares qpb::route over n = 1..129, m = 0..257 and the four
flag sets with the if-chains the C-ABI carried before, and walks batches of
0, 1, 4, 5 and 11 QPs in chunks of 4 over fake base addresses."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "route", "route_check.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def host_compiler():
    for cxx in (os.environ.get("CXX"), "g++", "clang++", "c++", "/opt/rocm/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_route_table_and_chunk_walker(tmp_path):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "route_check")
    inc = ["-I", os.path.join(ROOT, "embedded-qp-solver_amd", "csrc"), "-I", os.path.join(ROOT, "include")]
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *SAN, *inc, SRC, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert "runtime error:" not in out and "AddressSanitizer" not in out, out[-4000:]
    assert r.returncode == 0, out[-4000:]
    assert r.stdout.strip().endswith("route_check ok")
