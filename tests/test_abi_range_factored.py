"""CPU tests of the boundary of qpb_solve_range_factored (in the style of
test_abi_factored.py): the two entry points are exported, the launchers stay
hidden, and every argument error is returned before any device work, each with
its code, in qpb.h's order."""
import ctypes
import os
import subprocess

from conftest import ROOT

LIB = os.environ.get("QPB_LIB", os.path.join(ROOT, "embedded-qp-solver_amd", "lib", "libqpb.so"))
INVALID, UNSUPPORTED, NO_DEVICE = -1, -2, -4
FLAG_DIAG_L2, FLAG_MIXED, FLAG_DIAG_WAVE = 1, 32, 256
# fac, f, bl, bu, x, lam, active, lower, status, iters
F_, FF_, BL_, BU_, X_, LAM_, ACT_, LOW_, ST_, IT_ = range(10)


class Desc(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("m", ctypes.c_int32), ("batch", ctypes.c_int64),
                ("max_iter", ctypes.c_int32), ("flags", ctypes.c_int32), ("feas_tol", ctypes.c_double)]


def _lib():
    lib = ctypes.CDLL(LIB)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.qpb_last_error.restype = ctypes.c_char_p
    lib.qpb_solve_range_factored.argtypes = [ctypes.POINTER(Desc), i32] + [vp] * 11
    lib.qpb_solve_range_factored_host.argtypes = [ctypes.POINTER(Desc), i32] + [vp] * 10
    return lib


def _device_present():
    if os.environ.get("QPB_SANITIZED"):
        return False
    import torch
    return torch.cuda.is_available()


def _aligned16(buf, off=0):
    """A pointer into `buf`, `off` bytes past a 16-byte boundary (fac must be on one)."""
    a = ctypes.addressof(buf)
    return ctypes.c_void_p(((a + 15) & ~15) + off)


def test_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {"qpb_solve_range_factored", "qpb_solve_range_factored_host"} <= syms
    # the buffer's own calls are the same ones: one buffer serves both solves
    assert {"qpb_factor_doubles", "qpb_factor_shared", "qpb_solve_factored"} <= syms
    assert not {s for s in syms if s.startswith("qpb_launch_")}


def test_argument_errors_without_gpu():
    lib = _lib()
    buf = ctypes.create_string_buffer(96)
    p = _aligned16(buf)
    null, ptrs = [None] * 10, [p] * 10
    err = lib.qpb_last_error
    calls = (("qpb_solve_range_factored",
              lambda d, meq, a: lib.qpb_solve_range_factored(ctypes.byref(d), meq, *a, None)),
             ("qpb_solve_range_factored_host",
              lambda d, meq, a: lib.qpb_solve_range_factored_host(ctypes.byref(d), meq, *a)))
    for name, call in calls:
        # 1. the descriptor's own rules come first, as in qpb_solve
        assert call(Desc(0, 0, 4, 0, 0, 0.0), 0, null) == INVALID, name
        assert call(Desc(129, 32, 4, 0, 0, 0.0), 0, null) == UNSUPPORTED, name
        assert call(Desc(16, 32, -1, 0, 0, 0.0), 0, null) == INVALID, name
        # 2. then meq < 0, before the flags
        assert call(Desc(16, 32, 4, 0, FLAG_MIXED, 0.0), -1, ptrs) == INVALID and b"meq < 0" in err(), name
        # ... and the flags, also above the size limit
        for flags in (FLAG_DIAG_L2, FLAG_MIXED, FLAG_DIAG_WAVE, 4):
            for n, m in ((16, 32), (48, 96)):
                assert call(Desc(n, m, 4, 0, flags, 0.0), 0, ptrs) == INVALID, (name, flags, n, m)
                assert b"flags" in err() and b"qpb_solve_range_factored" in err()
        # 3. then the size, before meq > m, batch == 0 and the pointers
        for n, m in ((33, 1), (33, 0), (32, 65), (16, 65), (33, 40), (128, 256)):
            for meq, batch, args in ((0, 4, ptrs), (0, 0, null), (m + 1, 4, null)):
                assert call(Desc(n, m, batch, 0, 0, 0.0), meq, args) == UNSUPPORTED, (name, n, m)
                assert b"n<=32" in err() and b"m<=64" in err()
        # 4. then meq > m, before batch == 0
        for n, m in ((16, 32), (20, 40), (5, 0)):
            for batch, args in ((4, ptrs), (0, null)):
                assert call(Desc(n, m, batch, 0, 0, 0.0), m + 1, args) == INVALID, (name, n, m)
                assert b"meq=" in err()
        # 5. batch 0 is a no-op before the pointers are looked at
        for n, m, meq in ((16, 32, 4), (20, 40, 0), (32, 64, 64), (3, 0, 0)):
            assert call(Desc(n, m, 0, 0, 0, 0.0), meq, null) == 0, (name, n, m)
        # 6. missing pointers: fac, f, x and status always (lower and iters may be NULL) ...
        for n, m in ((16, 32), (20, 33), (3, 0)):
            for k in (F_, FF_, X_, ST_):
                args = list(ptrs)
                args[k] = None
                assert call(Desc(n, m, 4, 0, 0, 0.0), 0, args) == INVALID and b"required" in err(), (name, n, m, k)
        # ... lam and active when m > 0 only, and one of bl and bu (not both)
        for k in (LAM_, ACT_):
            args = list(ptrs)
            args[k] = None
            assert call(Desc(16, 32, 4, 0, 0, 0.0), 2, args) == INVALID and b"required" in err(), (name, k)
            assert call(Desc(20, 33, 4, 0, 0, 0.0), 0, args) == INVALID, (name, k)
        args = list(ptrs)
        args[BL_] = args[BU_] = None
        assert call(Desc(16, 32, 4, 0, 0, 0.0), 0, args) == INVALID and b"at least one of bl and bu" in err(), name
        assert call(Desc(20, 40, 4, 0, 0, 0.0), 0, args) == INVALID, name
        # ... and a missing pointer is reported before the buffer's alignment
        args = [_aligned16(buf, 8)] + [p] * 9
        args[X_] = None
        assert call(Desc(16, 32, 4, 0, 0, 0.0), 0, args) == INVALID and b"required" in err(), name
    # 7. fac off a 16-byte boundary (device pointers: the host form copies the buffer), with and without rows
    for n, m in ((16, 32), (20, 40), (3, 0)):
        args = [_aligned16(buf, 8)] + [p] * 9
        d = Desc(n, m, 4, 0, 0, 0.0)
        assert lib.qpb_solve_range_factored(ctypes.byref(d), 0, *args, None) == INVALID, (n, m)
        assert b"16-byte aligned" in err()
    if not _device_present():
        # 8. a valid call with no device fails loudly last: lower and iters NULL, one side NULL
        for n, m, meq in ((16, 32, 0), (16, 32, 4), (16, 16, 3), (20, 40, 3), (32, 64, 0)):
            for side in (None, BL_, BU_):
                args = list(ptrs)
                args[IT_] = args[LOW_] = None
                if side is not None:
                    args[side] = None
                d = Desc(n, m, 4, 0, 0, 0.0)
                assert lib.qpb_solve_range_factored(ctypes.byref(d), meq, *args, None) == NO_DEVICE, (n, m, side)
                assert b"no HIP device" in err()
                assert lib.qpb_solve_range_factored_host(ctypes.byref(d), meq, *args) == NO_DEVICE, (n, m, side)
        # m == 0: no rows, nothing but fac, f, x and status
        args = list(null)
        args[F_] = args[FF_] = args[X_] = args[ST_] = p
        assert lib.qpb_solve_range_factored(ctypes.byref(Desc(3, 0, 4, 0, 0, 0.0)), 0, *args, None) == NO_DEVICE


def test_version_names_the_range_factored_forms_beside_the_old_ones():
    lib = _lib()
    lib.qpb_version.restype = ctypes.c_char_p
    v = lib.qpb_version().decode()
    assert v.startswith("qpb 0.14 ")
    tokens = [t.strip() for t in v[v.index("(") + 1:].split(";")]
    assert any(t.startswith("gi_rfact v1.0:") for t in tokens)
    for old in ("gfx950", "gi_dense v11.7", "gi_box v2.2", "gi_wave v6.7", "gi_gram v4.5", "ref v6", "gi_eq v1.0",
                "kkt_bwd v1.1", "kkt_bwd_box v1.0", "gi_shared v1.0", "kkt_bwd_sum v1.0", "gi_range v1.0",
                "gi_fact v1.0"):
        assert any(t.startswith(old) for t in tokens), old


def test_python_binding_has_the_calls():
    if os.environ.get("QPB_SANITIZED"):
        return  # imports torch
    import inspect

    import qpb
    import qpb.diff
    for name in ("solve_range_factored", "solve_range_factored_host"):
        assert callable(getattr(qpb, name)), name
    sig = inspect.signature(qpb.solve_range_factored)
    assert list(sig.parameters)[:5] == ["F", "f", "bl", "bu", "meq"] and sig.parameters["meq"].default == 0
    assert {"max_iter", "feas_tol", "out", "stream"} <= set(sig.parameters)
    assert inspect.signature(qpb.diff.solve_range).parameters["prefactor"].default is False
