"""The workspace cache (csrc/qpb_workspace.hip) on the host, without a GPU.

tests/workspace/ws_check.cpp (its own main) links the unmodified source,
compiled host-only, against stubs of the six HIP calls it makes, and is built
twice -- under ThreadSanitizer and under AddressSanitizer + UBSan -- and run
directly (no preloaded runtime).  It checks buffer identity (one buffer per
device and stream, grown in 1 MiB steps, never shrunk, freed on the stream and
device it was allocated on), both release calls, six threads over three streams
with releases interleaved (the entry lock and the dead-entry retry), and a
failing allocation."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "workspace", "ws_check.cpp")
CACHE = os.path.join(ROOT, "embedded-qp-solver_amd", "csrc", "qpb_workspace.hip")
INC = ["-I", os.path.join(ROOT, "embedded-qp-solver_amd", "csrc"), "-I", os.path.join(ROOT, "include")]
SANITIZERS = {"tsan": ["-fsanitize=thread"],
              "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}


def _tools():
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc")) or shutil.which("/opt/rocm/bin/hipcc")
    clangxx = shutil.which("/opt/rocm/llvm/bin/clang++") or shutil.which("/opt/rocm/lib/llvm/bin/clang++")
    return hipcc, clangxx


def build_ws_check(tmp_path, san, cache_src=CACHE):
    """Both sources host-only with hipcc, the sanitizer on the host side;
    linked by ROCm's clang++ with the same sanitizer and no HIP library."""
    hipcc, clangxx = _tools()
    host = [f for s in SANITIZERS[san] + ["-fno-omit-frame-pointer"] for f in ("-Xarch_host", s)]
    objs = []
    for src in (cache_src, SRC):
        obj = str(tmp_path / (os.path.basename(src) + f".{san}.o"))
        r = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++20", "-O1", "-g", "-Wall", *host, *INC,
                            "-c", src, "-o", obj], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        objs.append(obj)
    exe = str(tmp_path / f"ws_check_{san}")
    r = subprocess.run([clangxx, *SANITIZERS[san], *objs, "-pthread", "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("san", list(SANITIZERS))
def test_workspace_cache_on_host(tmp_path, san):
    if None in _tools():
        pytest.skip("no hipcc / ROCm clang++")
    exe = build_ws_check(tmp_path, san)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    print(out[-2000:])
    for word in ("ThreadSanitizer", "AddressSanitizer", "runtime error:"):
        assert word not in out, out[-4000:]
    assert r.returncode == 0, out[-4000:]
    assert r.stdout.strip().endswith("ws_check ok")
