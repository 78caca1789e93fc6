"""CPU tests of qpb_solve_backward_dual's boundary (in the style of
test_abi_backward.py): the two entry points are exported, the launcher stays
hidden, and every argument error is returned before any device work, each with
its code, in qpb.h's order -- with glam given, NULL and odd (never read)."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT

LIB = os.environ.get("QPB_LIB", os.path.join(ROOT, "embedded-qp-solver_amd", "lib", "libqpb.so"))
INVALID, UNSUPPORTED, NO_DEVICE = -1, -2, -4
FLAG_DIAG_L2, FLAG_MIXED, FLAG_DIAG_WAVE = 1, 32, 256
# H, A, x, lam, active, status, gx, glam, gH, gf, gA, gb
H_, A_, X_, LAM_, ACT_, ST_, GX_, GL_, GH_, GF_, GA_, GB_ = range(12)


class Desc(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("m", ctypes.c_int32), ("batch", ctypes.c_int64),
                ("max_iter", ctypes.c_int32), ("flags", ctypes.c_int32), ("feas_tol", ctypes.c_double)]


def _lib():
    lib = ctypes.CDLL(LIB)
    vp = ctypes.c_void_p
    lib.qpb_last_error.restype = ctypes.c_char_p
    lib.qpb_solve_backward_dual.argtypes = [ctypes.POINTER(Desc), ctypes.c_int32] + [vp] * 13
    lib.qpb_solve_backward_dual_host.argtypes = [ctypes.POINTER(Desc), ctypes.c_int32] + [vp] * 12
    return lib


def _device_present():
    if os.environ.get("QPB_SANITIZED"):
        return False
    import torch
    return torch.cuda.is_available()


def test_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {"qpb_solve_backward_dual", "qpb_solve_backward_dual_host"} <= syms
    assert not {s for s in syms if s.startswith("qpb_launch_")}


def _calls(lib):
    """Both entry points with the same (desc, shared, twelve array pointers)."""
    return (("qpb_solve_backward_dual", lambda d, sh, a: lib.qpb_solve_backward_dual(ctypes.byref(d), sh, *a, None)),
            ("qpb_solve_backward_dual_host", lambda d, sh, a: lib.qpb_solve_backward_dual_host(ctypes.byref(d), sh, *a)))


def test_argument_errors_without_gpu():
    lib = _lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 1)  # misaligned: nothing is read before the checks are through
    null = [None] * 12
    for glam in (p, None, odd):
        ptrs = [p] * 12
        ptrs[GL_] = glam
        for name, call in _calls(lib):
            for shared in (0, 1, 2, 3):
                # the descriptor's own rules come first, as in qpb_solve
                assert call(Desc(0, 0, 4, 0, 0, 0.0), shared, null) == INVALID, name
                assert call(Desc(129, 32, 4, 0, 0, 0.0), shared, null) == UNSUPPORTED, name
                assert call(Desc(16, 32, -1, 0, 0, 0.0), shared, null) == INVALID, name
                # then the flags, also above the size limit
                for flags in (FLAG_DIAG_L2, FLAG_MIXED, FLAG_DIAG_WAVE, 4):
                    for n, m in ((16, 32), (48, 96)):
                        assert call(Desc(n, m, 4, 0, flags, 0.0), shared, ptrs) == INVALID, (name, flags, n, m)
                        assert b"flags" in lib.qpb_last_error()
                # then the size, before batch == 0 and the pointers
                for n, m in ((33, 0), (16, 65), (129, 32), (32, 65), (128, 256)):
                    for batch, args in ((4, ptrs), (0, null), (4, null)):
                        assert call(Desc(n, m, batch, 0, 0, 0.0), shared, args) == UNSUPPORTED, (name, n, m, batch)
                        if n <= 128:  # (above 128 the descriptor's own message)
                            assert b"n<=32" in lib.qpb_last_error() and b"m<=64" in lib.qpb_last_error()
                # batch 0 is a no-op before the pointers are looked at
                for n, m in ((16, 32), (20, 40), (32, 64), (3, 0)):
                    assert call(Desc(n, m, 0, 0, 0, 0.0), shared, null) == 0, (name, n, m)
                # missing pointers, at both kernel classes: H, x and gx always ...
                for n, m in ((16, 32), (20, 33), (3, 0)):
                    for k in (H_, X_, GX_):
                        args = list(ptrs)
                        args[k] = None
                        assert call(Desc(n, m, 4, 0, 0, 0.0), shared, args) == INVALID, (name, n, m, k)
                # ... A, lam and active when m > 0 only
                for k in (A_, LAM_, ACT_):
                    args = list(ptrs)
                    args[k] = None
                    assert call(Desc(16, 32, 4, 0, 0, 0.0), shared, args) == INVALID, (name, k)
                    assert call(Desc(20, 33, 4, 0, 0, 0.0), shared, args) == INVALID, (name, k)
                # ... and at least one output (with m == 0, gA and gb are ignored and do not count)
                args = list(ptrs)
                args[GH_] = args[GF_] = args[GA_] = args[GB_] = None
                assert call(Desc(16, 32, 4, 0, 0, 0.0), shared, args) == INVALID, name
                args[GA_] = args[GB_] = p
                assert call(Desc(3, 0, 4, 0, 0, 0.0), shared, args) == INVALID, name
            # a stray bit of `shared` is an argument error after the flags' and before the size's
            for shared in (4, 7, -1):
                assert call(Desc(16, 32, 4, 0, 0, 0.0), shared, ptrs) == INVALID, (name, shared)
                assert b"shared" in lib.qpb_last_error()
                assert call(Desc(33, 0, 4, 0, 0, 0.0), shared, ptrs) == INVALID, (name, shared)
                assert call(Desc(16, 32, 4, 0, FLAG_MIXED, 0.0), shared, ptrs) == INVALID
                assert b"flags" in lib.qpb_last_error()
    if not _device_present():
        # a valid call with no device fails loudly last
        ptrs = [p] * 12
        for n, m in ((16, 32), (20, 40), (32, 64)):
            d = Desc(n, m, 4, 0, 0, 0.0)
            for shared in (0, 3):
                for glam in (p, None):
                    for only in (GH_, GF_, GA_, GB_):
                        args = list(ptrs)
                        args[ST_], args[GL_] = None, glam
                        for k in (GH_, GF_, GA_, GB_):
                            args[k] = p if k == only else None
                        assert lib.qpb_solve_backward_dual(ctypes.byref(d), shared, *args, None) == NO_DEVICE
                        assert b"no HIP device" in lib.qpb_last_error()
                        assert lib.qpb_solve_backward_dual_host(ctypes.byref(d), shared, *args) == NO_DEVICE


def test_version_is_unchanged():
    lib = _lib()
    lib.qpb_version.restype = ctypes.c_char_p
    assert lib.qpb_version().decode().startswith("qpb 0.14 ")


def test_python_binding_has_the_calls_and_checks_its_arguments():
    if os.environ.get("QPB_SANITIZED"):
        return  # imports torch
    import numpy as np
    import qpb
    import qpb.diff
    torch = __import__("torch")
    assert callable(qpb.solve_backward_dual) and callable(qpb.solve_backward_dual_host) and callable(qpb.solve_tangent)
    assert issubclass(qpb.diff.DualQPFunction, torch.autograd.Function)
    assert issubclass(qpb.diff.RangeDualQPFunction, torch.autograd.Function)
    # the device wrappers refuse host tensors before any call into the library
    B, n, m = 3, 4, 5
    z = lambda *s: torch.zeros(s, dtype=torch.float64)  # noqa: E731
    sol = qpb.Solution(z(B, n), z(B, m), torch.zeros((B, 1), dtype=torch.int32), None, None)
    with pytest.raises(ValueError, match="CUDA"):
        qpb.solve_backward_dual(z(B, n, n), z(B, m, n), sol, z(B, n), z(B, m))
    with pytest.raises(ValueError, match="CUDA"):
        qpb.solve_tangent(z(B, n, n), z(B, m, n), sol, z(B, n), z(B, m))
    with pytest.raises(ValueError, match="needs A and b"):
        qpb.diff.solve_dual(z(B, n, n), z(B, n), None, None)
    # the host wrapper checks shapes and `need` before the library is called
    hs = qpb.Solution(np.zeros((B, n)), np.zeros((B, m)), np.zeros((B, 1), np.uint32), None, None)
    with pytest.raises(ValueError, match="shape mismatch"):
        qpb.solve_backward_dual_host(np.zeros((B, n, n)), np.zeros((B, m, n)), hs, np.zeros((B, n)), np.zeros((B, m + 1)))
    with pytest.raises(ValueError, match="need"):
        qpb.solve_backward_dual_host(np.zeros((B, n, n)), np.zeros((B, m, n)), hs, np.zeros((B, n)), np.zeros((B, m)),
                                     need=("x",))
    # errors of the library come back as QPBError with the code
    with pytest.raises(qpb.QPBError) as e:
        qpb.solve_backward_dual_host(np.zeros((B, 33, 33)), None, qpb.Solution(np.zeros((B, 33)), None, None, None, None),
                                     np.zeros((B, 33)), None)
    assert e.value.code == qpb.ERR_UNSUPPORTED
