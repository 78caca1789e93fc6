"""CPU tests of qpb_solve_eq's boundary (in the style of test_abi.py): the two
entry points are exported, the launchers stay hidden, and every argument error
is returned before any device work, each with its code."""
import ctypes
import os
import subprocess

from conftest import ROOT

LIB = os.environ.get("QPB_LIB", os.path.join(ROOT, "embedded-qp-solver_amd", "lib", "libqpb.so"))
INVALID, UNSUPPORTED, NO_DEVICE = -1, -2, -4
FLAG_DIAG_L2, FLAG_MIXED, FLAG_DIAG_WAVE = 1, 32, 256


class Desc(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("m", ctypes.c_int32), ("batch", ctypes.c_int64),
                ("max_iter", ctypes.c_int32), ("flags", ctypes.c_int32), ("feas_tol", ctypes.c_double)]


def _lib():
    lib = ctypes.CDLL(LIB)
    vp = ctypes.c_void_p
    lib.qpb_last_error.restype = ctypes.c_char_p
    lib.qpb_solve_eq.argtypes = [ctypes.POINTER(Desc), ctypes.c_int32] + [vp] * 10
    lib.qpb_solve_eq_host.argtypes = [ctypes.POINTER(Desc), ctypes.c_int32] + [vp] * 9
    return lib


def _device_present():
    if os.environ.get("QPB_SANITIZED"):
        return False
    import torch
    return torch.cuda.is_available()


def test_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {"qpb_solve_eq", "qpb_solve_eq_host"} <= syms
    assert not {s for s in syms if s.startswith("qpb_launch_")}


def _calls(lib):
    """Both entry points with the same (desc, meq, nine array pointers)."""
    return (("qpb_solve_eq", lambda d, meq, a: lib.qpb_solve_eq(ctypes.byref(d), meq, *a, None)),
            ("qpb_solve_eq_host", lambda d, meq, a: lib.qpb_solve_eq_host(ctypes.byref(d), meq, *a)))


def test_argument_errors_without_gpu():
    lib = _lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    null, ptrs = [None] * 9, [p] * 9
    for name, call in _calls(lib):
        # the descriptor's own rules come first, as in qpb_solve
        assert call(Desc(0, 0, 4, 0, 0, 0.0), 0, null) == INVALID, name
        assert call(Desc(129, 32, 4, 0, 0, 0.0), 0, null) == UNSUPPORTED, name
        assert call(Desc(16, 32, -1, 0, 0, 0.0), 4, null) == INVALID, name
        # meq outside 0 .. m
        assert call(Desc(16, 32, 4, 0, 0, 0.0), -1, ptrs) == INVALID, name
        assert call(Desc(16, 32, 4, 0, 0, 0.0), 33, ptrs) == INVALID, name
        assert b"meq" in lib.qpb_last_error()
        assert call(Desc(20, 40, 4, 0, 0, 0.0), 41, ptrs) == INVALID, name
        # the flags select nothing here, whatever meq
        for flags in (FLAG_DIAG_L2, FLAG_MIXED, FLAG_DIAG_WAVE, 4):
            for meq in (0, 4):
                assert call(Desc(16, 32, 4, 0, flags, 0.0), meq, ptrs) == INVALID, (name, flags, meq)
            assert b"flags" in lib.qpb_last_error()
        # meq > 0 above the two wavefront-level classes: unsupported, and the message names the limit
        for n, m in ((33, 0), (32, 65), (16, 65), (33, 40), (128, 256)):
            assert call(Desc(n, m, 4, 0, 0, 0.0), 1, ptrs) == UNSUPPORTED, (name, n, m)
            assert b"n<=32" in lib.qpb_last_error() and b"m<=64" in lib.qpb_last_error()
        # batch 0 is a no-op, with or without equalities
        for meq in (0, 4):
            assert call(Desc(16, 32, 0, 0, 0, 0.0), meq, null) == 0, name
        assert call(Desc(48, 96, 0, 0, 0, 0.0), 0, null) == 0, name
    # the pointer rules are qpb_solve's (iters may be NULL), at both kernel classes
    for n, m in ((16, 32), (20, 33)):
        for k in range(8):  # H, f, A, b, x, lam, active, status
            args = [p] * 9
            args[k] = None
            assert lib.qpb_solve_eq(ctypes.byref(Desc(n, m, 4, 0, 0, 0.0)), 3, *args, None) == INVALID, (n, m, k)
            assert lib.qpb_solve_eq_host(ctypes.byref(Desc(n, m, 4, 0, 0, 0.0)), 3, *args) == INVALID, (n, m, k)
    if not _device_present():
        # a valid call with no device fails loudly, meq = m and iters = NULL included
        for n, m, meq in ((16, 32, 4), (20, 33, 5), (32, 64, 64), (48, 96, 0)):
            d = Desc(n, m, 4, 0, 0, 0.0)
            assert lib.qpb_solve_eq(ctypes.byref(d), meq, *([p] * 8), None, None) == NO_DEVICE, (n, m, meq)
            assert b"no HIP device" in lib.qpb_last_error()
            assert lib.qpb_solve_eq_host(ctypes.byref(d), meq, *([p] * 8), None) == NO_DEVICE, (n, m, meq)


def test_python_binding_has_the_calls():
    if os.environ.get("QPB_SANITIZED"):
        return  # imports torch
    import qpb
    assert callable(qpb.solve_eq) and callable(qpb.solve_eq_host)
    assert "gi_eq v1.0" in qpb.version() and "gi_dense v11.6" in qpb.version()
