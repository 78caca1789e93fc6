"""CPU tests of the boundary of qpb_solve_range (in the style of
test_abi_shared.py): the two entry points are exported, the launchers stay
hidden, and every argument error is returned before any device work, each with
its code, in qpb.h's order."""
import ctypes
import os
import subprocess

from conftest import ROOT

LIB = os.environ.get("QPB_LIB", os.path.join(ROOT, "embedded-qp-solver_amd", "lib", "libqpb.so"))
INVALID, UNSUPPORTED, NO_DEVICE = -1, -2, -4
FLAG_DIAG_L2, FLAG_MIXED, FLAG_DIAG_WAVE = 1, 32, 256
SHARED_H, SHARED_A = 1, 2
# H, f, A, bl, bu, x, lam, active, lower, status, iters
H_, F_, A_, BL_, BU_, X_, LAM_, ACT_, LOW_, ST_, IT_ = range(11)


class Desc(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("m", ctypes.c_int32), ("batch", ctypes.c_int64),
                ("max_iter", ctypes.c_int32), ("flags", ctypes.c_int32), ("feas_tol", ctypes.c_double)]


def _lib():
    lib = ctypes.CDLL(LIB)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.qpb_last_error.restype = ctypes.c_char_p
    lib.qpb_solve_range.argtypes = [ctypes.POINTER(Desc), i32, i32] + [vp] * 12
    lib.qpb_solve_range_host.argtypes = [ctypes.POINTER(Desc), i32, i32] + [vp] * 11
    return lib


def _device_present():
    if os.environ.get("QPB_SANITIZED"):
        return False
    import torch
    return torch.cuda.is_available()


def test_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {"qpb_solve_range", "qpb_solve_range_host"} <= syms
    assert not {s for s in syms if s.startswith("qpb_launch_")}


def _calls(lib):
    return (("qpb_solve_range", lambda d, meq, sh, a: lib.qpb_solve_range(ctypes.byref(d), meq, sh, *a, None)),
            ("qpb_solve_range_host", lambda d, meq, sh, a: lib.qpb_solve_range_host(ctypes.byref(d), meq, sh, *a)))


def test_argument_errors_without_gpu():
    lib = _lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    null, ptrs = [None] * 11, [p] * 11
    err = lib.qpb_last_error
    for name, call in _calls(lib):
        for sh in (0, 1, 2, 3):
            # the descriptor's own rules come first, as in qpb_solve
            assert call(Desc(0, 0, 4, 0, 0, 0.0), 0, sh, null) == INVALID, name
            assert call(Desc(129, 32, 4, 0, 0, 0.0), 0, sh, null) == UNSUPPORTED, name
            assert b"range" not in err()  # the descriptor's message, not this call's
            assert call(Desc(16, 32, -1, 0, 0, 0.0), 0, sh, null) == INVALID, name
            # then meq < 0, before the flags
            assert call(Desc(16, 32, 4, 0, FLAG_MIXED, 0.0), -1, sh, ptrs) == INVALID and b"meq < 0" in err(), name
            # then the flags, also above the size limit and with a bad `shared`
            for flags in (FLAG_DIAG_L2, FLAG_MIXED, FLAG_DIAG_WAVE, 4):
                for n, m in ((16, 32), (48, 96)):
                    assert call(Desc(n, m, 4, 0, flags, 0.0), 0, sh | 4, ptrs) == INVALID, (name, flags, n, m)
                    assert b"flags" in err()
        # then the bits of `shared`, before the size, meq > m and batch == 0
        for sh in (4, 7, 8, -1, 1 << 30):
            for n, m, meq, batch in ((16, 32, 0, 4), (48, 96, 0, 4), (16, 32, 33, 4), (16, 32, 0, 0)):
                assert call(Desc(n, m, batch, 0, 0, 0.0), meq, sh, null) == INVALID, (name, sh, n, m)
                assert b"QPB_SHARED_H" in err()
        # then the size, whatever is shared: the two wavefront-level classes only, a message that
        # names the call and the limit, before meq > m, batch == 0 and the pointers
        for sh in (0, 1, 2, 3):
            for n, m in ((33, 1), (1, 65), (32, 65), (16, 65), (33, 40), (128, 256), (33, 0)):
                for meq, batch, args in ((0, 4, ptrs), (0, 0, null), (m + 1, 4, null)):
                    assert call(Desc(n, m, batch, 0, 0, 0.0), meq, sh, args) == UNSUPPORTED, (name, n, m, sh)
                    assert b"range" in err() and b"n<=32" in err() and b"m<=64" in err()
        # then meq > m
        for sh in (0, 1, 2, 3):
            for n, m in ((16, 32), (20, 40), (5, 0)):
                for batch, args in ((4, ptrs), (0, null)):
                    assert call(Desc(n, m, batch, 0, 0, 0.0), m + 1, sh, args) == INVALID, (name, n, m, sh)
                    assert b"meq=" in err()
        # batch 0 is a no-op before the pointers are looked at
        for sh in (0, 1, 2, 3):
            for n, m, meq in ((16, 32, 4), (20, 40, 0), (32, 64, 64), (3, 0, 0)):
                assert call(Desc(n, m, 0, 0, 0, 0.0), meq, sh, null) == 0, (name, n, m, sh)
        # missing pointers: H, f, x and status always (lower and iters may be NULL) ...
        for sh in (0, 1, 2, 3):
            for n, m in ((16, 32), (20, 33), (3, 0)):
                for k in (H_, F_, X_, ST_):
                    args = list(ptrs)
                    args[k] = None
                    assert call(Desc(n, m, 4, 0, 0, 0.0), 0, sh, args) == INVALID, (name, n, m, k)
                    assert b"required" in err()
            # ... A, lam and active when m > 0 only
            for k in (A_, LAM_, ACT_):
                args = list(ptrs)
                args[k] = None
                assert call(Desc(16, 32, 4, 0, 0, 0.0), 2, sh, args) == INVALID, (name, k)
                assert call(Desc(20, 33, 4, 0, 0, 0.0), 0, sh, args) == INVALID, (name, k)
            # ... and at least one of bl and bu
            args = list(ptrs)
            args[BL_] = args[BU_] = None
            for n, m in ((16, 32), (20, 33)):
                assert call(Desc(n, m, 4, 0, 0, 0.0), 0, sh, args) == INVALID, (name, n, m)
                assert b"at least one of bl and bu" in err()
    if not _device_present():
        # a valid call with no device fails loudly last: either bound alone, lower and iters NULL
        for sh in (0, 1, 2, 3):
            for n, m, meq in ((16, 32, 0), (16, 32, 4), (20, 40, 3), (32, 64, 0), (1, 1, 1)):
                for drop in ((), (BL_,), (BU_,), (LOW_, IT_)):
                    args = list(ptrs)
                    for k in drop:
                        args[k] = None
                    d = Desc(n, m, 4, 0, 0, 0.0)
                    assert lib.qpb_solve_range(ctypes.byref(d), meq, sh, *args, None) == NO_DEVICE, (n, m, sh, drop)
                    assert b"no HIP device" in err()
                    assert lib.qpb_solve_range_host(ctypes.byref(d), meq, sh, *args) == NO_DEVICE, (n, m, sh, drop)
        # m == 0: the call is qpb_solve, with its pointers only
        args = list(ptrs)
        args[A_] = args[BL_] = args[BU_] = args[LAM_] = args[ACT_] = args[LOW_] = None
        assert lib.qpb_solve_range(ctypes.byref(Desc(3, 0, 4, 0, 0, 0.0)), 0, 3, *args, None) == NO_DEVICE


def test_version_names_the_range_kernels_beside_the_old_ones():
    lib = _lib()
    lib.qpb_version.restype = ctypes.c_char_p
    v = lib.qpb_version().decode()
    assert v.startswith("qpb 0.14 ")
    tokens = [t.strip() for t in v[v.index("(") + 1:].split(";")]
    assert any(t.startswith("gi_range v1.0:") for t in tokens)
    for old in ("gfx950", "gi_dense v11.7", "gi_box v2.2", "gi_wave v6.7", "gi_gram v4.5", "ref v6", "gi_eq v1.0",
                "kkt_bwd v1.1", "kkt_bwd_box v1.0", "gi_shared v1.0", "kkt_bwd_sum v1.0"):
        assert any(t.startswith(old) for t in tokens), old
    assert "gi_dense v11.6" in v


def test_python_binding_has_the_calls():
    if os.environ.get("QPB_SANITIZED"):
        return  # imports torch
    import qpb
    for name in ("solve_range", "solve_range_host"):
        assert callable(getattr(qpb, name)), name
    assert qpb.RangeSolution._fields == ("x", "lam", "active", "lower", "status", "iters")
    assert qpb.Solution._fields == ("x", "lam", "active", "status", "iters")
    import qpb.diff
    assert callable(qpb.diff.solve_range)
