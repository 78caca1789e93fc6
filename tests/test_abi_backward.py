"""CPU tests of qpb_solve_backward's boundary (in the style of test_abi_eq.py):
the two entry points are exported, the launcher stays hidden, and every
argument error is returned before any device work, each with its code, in
qpb.h's order."""
import ctypes
import os
import subprocess

from conftest import ROOT

LIB = os.environ.get("QPB_LIB", os.path.join(ROOT, "embedded-qp-solver_amd", "lib", "libqpb.so"))
INVALID, UNSUPPORTED, NO_DEVICE = -1, -2, -4
FLAG_DIAG_L2, FLAG_MIXED, FLAG_DIAG_WAVE = 1, 32, 256
# H, A, x, lam, active, status, gx, gH, gf, gA, gb
H_, A_, X_, LAM_, ACT_, ST_, GX_, GH_, GF_, GA_, GB_ = range(11)


class Desc(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("m", ctypes.c_int32), ("batch", ctypes.c_int64),
                ("max_iter", ctypes.c_int32), ("flags", ctypes.c_int32), ("feas_tol", ctypes.c_double)]


def _lib():
    lib = ctypes.CDLL(LIB)
    vp = ctypes.c_void_p
    lib.qpb_last_error.restype = ctypes.c_char_p
    lib.qpb_solve_backward.argtypes = [ctypes.POINTER(Desc)] + [vp] * 12
    lib.qpb_solve_backward_host.argtypes = [ctypes.POINTER(Desc)] + [vp] * 11
    return lib


def _device_present():
    if os.environ.get("QPB_SANITIZED"):
        return False
    import torch
    return torch.cuda.is_available()


def test_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {"qpb_solve_backward", "qpb_solve_backward_host"} <= syms
    assert not {s for s in syms if s.startswith("qpb_launch_")}


def _calls(lib):
    """Both entry points with the same (desc, eleven array pointers)."""
    return (("qpb_solve_backward", lambda d, a: lib.qpb_solve_backward(ctypes.byref(d), *a, None)),
            ("qpb_solve_backward_host", lambda d, a: lib.qpb_solve_backward_host(ctypes.byref(d), *a)))


def test_argument_errors_without_gpu():
    lib = _lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    null, ptrs = [None] * 11, [p] * 11
    for name, call in _calls(lib):
        # the descriptor's own rules come first, as in qpb_solve
        assert call(Desc(0, 0, 4, 0, 0, 0.0), null) == INVALID, name
        assert call(Desc(129, 32, 4, 0, 0, 0.0), null) == UNSUPPORTED, name
        assert call(Desc(16, 32, -1, 0, 0, 0.0), null) == INVALID, name
        # then the flags: none selects anything here, also above the size limit
        for flags in (FLAG_DIAG_L2, FLAG_MIXED, FLAG_DIAG_WAVE, 4):
            for n, m in ((16, 32), (48, 96)):
                assert call(Desc(n, m, 4, 0, flags, 0.0), ptrs) == INVALID, (name, flags, n, m)
                assert b"flags" in lib.qpb_last_error()
        # then the size: the two wavefront-level classes only, before batch == 0 and the pointers
        for n, m in ((33, 0), (32, 65), (16, 65), (33, 40), (128, 256)):
            for batch, args in ((4, ptrs), (0, null), (4, null)):
                assert call(Desc(n, m, batch, 0, 0, 0.0), args) == UNSUPPORTED, (name, n, m, batch)
                assert b"n<=32" in lib.qpb_last_error() and b"m<=64" in lib.qpb_last_error()
        # batch 0 is a no-op before the pointers are looked at
        for n, m in ((16, 32), (20, 40), (32, 64), (3, 0)):
            assert call(Desc(n, m, 0, 0, 0, 0.0), null) == 0, (name, n, m)
        # missing pointers, at both kernel classes: H, x and gx always ...
        for n, m in ((16, 32), (20, 33), (3, 0)):
            for k in (H_, X_, GX_):
                args = list(ptrs)
                args[k] = None
                assert call(Desc(n, m, 4, 0, 0, 0.0), args) == INVALID, (name, n, m, k)
        # ... A, lam and active when m > 0 only
        for k in (A_, LAM_, ACT_):
            args = list(ptrs)
            args[k] = None
            assert call(Desc(16, 32, 4, 0, 0, 0.0), args) == INVALID, (name, k)
            assert call(Desc(20, 33, 4, 0, 0, 0.0), args) == INVALID, (name, k)
        # ... and at least one output (with m == 0, gA and gb are ignored and do not count)
        args = list(ptrs)
        args[GH_] = args[GF_] = args[GA_] = args[GB_] = None
        assert call(Desc(16, 32, 4, 0, 0, 0.0), args) == INVALID, name
        args[GA_] = args[GB_] = p
        assert call(Desc(3, 0, 4, 0, 0, 0.0), args) == INVALID, name
    if not _device_present():
        # a valid call with no device fails loudly last: status NULL, any one output, A .. active NULL at m = 0
        for n, m in ((16, 32), (20, 40), (32, 64)):
            d = Desc(n, m, 4, 0, 0, 0.0)
            for only in (GH_, GF_, GA_, GB_):
                args = list(ptrs)
                args[ST_] = None
                for k in (GH_, GF_, GA_, GB_):
                    args[k] = p if k == only else None
                assert lib.qpb_solve_backward(ctypes.byref(d), *args, None) == NO_DEVICE, (n, m, only)
                assert b"no HIP device" in lib.qpb_last_error()
                assert lib.qpb_solve_backward_host(ctypes.byref(d), *args) == NO_DEVICE, (n, m, only)
        args = list(ptrs)
        args[A_] = args[LAM_] = args[ACT_] = args[GA_] = args[GB_] = None
        assert lib.qpb_solve_backward(ctypes.byref(Desc(3, 0, 4, 0, 0, 0.0)), *args, None) == NO_DEVICE


def test_version_names_the_backward_kernels():
    lib = _lib()
    lib.qpb_version.restype = ctypes.c_char_p
    v = lib.qpb_version().decode()
    assert v.startswith("qpb 0.14 ") and "kkt_bwd v1.1" in v
    assert "gi_eq v1.0" in v and "gi_dense v11.6" in v


def test_python_binding_has_the_calls():
    if os.environ.get("QPB_SANITIZED"):
        return  # imports torch
    import qpb
    assert callable(qpb.solve_backward) and callable(qpb.solve_backward_host)
    import qpb.diff
    assert callable(qpb.diff.solve) and issubclass(qpb.diff.QPFunction, __import__("torch").autograd.Function)
