"""CPU tests of the boundary of qpb_factor_doubles, qpb_factor_shared and
qpb_solve_factored (in the style of test_abi_shared.py): the five entry points
are exported, the launchers stay hidden, the size of a factor buffer is host
arithmetic, and every argument error is returned before any device work, each
with its code, in qpb.h's order."""
import ctypes
import os
import subprocess

from conftest import ROOT

LIB = os.environ.get("QPB_LIB", os.path.join(ROOT, "embedded-qp-solver_amd", "lib", "libqpb.so"))
INVALID, UNSUPPORTED, NO_DEVICE = -1, -2, -4
FLAG_DIAG_L2, FLAG_MIXED, FLAG_DIAG_WAVE = 1, 32, 256
# solve: fac, f, b, x, lam, active, status, iters
SF_, SFF_, SB_, SX_, SLAM_, SACT_, SST_, SIT_ = range(8)
# factor: H, A, fac, fstatus
FH_, FA_, FF_, FS_ = range(4)


class Desc(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("m", ctypes.c_int32), ("batch", ctypes.c_int64),
                ("max_iter", ctypes.c_int32), ("flags", ctypes.c_int32), ("feas_tol", ctypes.c_double)]


def _lib():
    lib = ctypes.CDLL(LIB)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.qpb_last_error.restype = ctypes.c_char_p
    lib.qpb_factor_doubles.argtypes = [i32, i32]
    lib.qpb_factor_doubles.restype = ctypes.c_int64
    lib.qpb_factor_shared.argtypes = [i32, i32] + [vp] * 5
    lib.qpb_factor_shared_host.argtypes = [i32, i32] + [vp] * 4
    lib.qpb_solve_factored.argtypes = [ctypes.POINTER(Desc), i32] + [vp] * 9
    lib.qpb_solve_factored_host.argtypes = [ctypes.POINTER(Desc), i32] + [vp] * 8
    return lib


def _device_present():
    if os.environ.get("QPB_SANITIZED"):
        return False
    import torch
    return torch.cuda.is_available()


def _aligned16(buf):
    """A pointer into `buf` on a 16-byte boundary (fac must be)."""
    a = ctypes.addressof(buf)
    return ctypes.c_void_p((a + 15) & ~15)


def test_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {"qpb_factor_doubles", "qpb_factor_shared", "qpb_factor_shared_host", "qpb_solve_factored",
            "qpb_solve_factored_host"} <= syms
    assert not {s for s in syms if s.startswith("qpb_launch_")}


def test_factor_doubles():
    lib = _lib()
    err = lib.qpb_last_error
    for n in (1, 5, 16, 17, 32):
        last = 0
        for m in range(0, 65):
            k = lib.qpb_factor_doubles(n, m)
            # positive, non-decreasing in m, and room for L, D and the copy of A at least
            assert k > 0 and k >= last, (n, m, k, last)
            assert k >= n * (n + 1) // 2 + 2 * m * n, (n, m, k)
            last = k
    assert lib.qpb_factor_doubles(33, 0) == UNSUPPORTED and b"n<=32" in err() and b"m<=64" in err()
    assert lib.qpb_factor_doubles(16, 65) == UNSUPPORTED
    assert lib.qpb_factor_doubles(0, 0) == INVALID
    assert lib.qpb_factor_doubles(1, -1) == INVALID
    assert lib.qpb_factor_doubles(0, 65) == INVALID  # the shape's own rules before the size


def test_factor_argument_errors_without_gpu():
    lib = _lib()
    buf = ctypes.create_string_buffer(96)
    p = _aligned16(buf)
    null, ptrs = [None] * 4, [p] * 4
    err = lib.qpb_last_error
    calls = (("qpb_factor_shared", lambda n, m, a: lib.qpb_factor_shared(n, m, *a, None)),
             ("qpb_factor_shared_host", lambda n, m, a: lib.qpb_factor_shared_host(n, m, *a)))
    for name, call in calls:
        # the shape first, as a descriptor's
        assert call(0, 0, null) == INVALID, name
        assert call(16, -1, ptrs) == INVALID, name
        assert call(0, 65, ptrs) == INVALID, name
        # then the size, before the pointers
        for n, m in ((33, 0), (33, 1), (16, 65), (32, 65), (128, 256)):
            for args in (null, ptrs):
                assert call(n, m, args) == UNSUPPORTED, (name, n, m)
                assert b"factored kernels" in err() and b"n<=32" in err() and b"m<=64" in err()
        # then the pointers: H and fac always (fstatus may be NULL), A when m > 0 only
        for n, m in ((16, 32), (20, 40), (3, 0)):
            for k in (FH_, FF_):
                args = list(ptrs)
                args[k] = None
                assert call(n, m, args) == INVALID and b"required" in err(), (name, n, m, k)
        args = list(ptrs)
        args[FA_] = None
        assert call(16, 32, args) == INVALID and b"A is required" in err(), name
        assert call(20, 33, args) == INVALID, name
    if not _device_present():
        # a valid call with no device fails loudly last: fstatus NULL, A NULL at m == 0
        for n, m in ((16, 32), (5, 9), (20, 40), (32, 64)):
            args = list(ptrs)
            args[FS_] = None
            assert lib.qpb_factor_shared(n, m, *args, None) == NO_DEVICE, (n, m)
            assert b"no HIP device" in err()
            assert lib.qpb_factor_shared_host(n, m, *args) == NO_DEVICE, (n, m)
        assert lib.qpb_factor_shared(3, 0, p, None, p, None, None) == NO_DEVICE


def test_solve_argument_errors_without_gpu():
    lib = _lib()
    buf = ctypes.create_string_buffer(96)
    p = _aligned16(buf)
    null, ptrs = [None] * 8, [p] * 8
    err = lib.qpb_last_error
    calls = (("qpb_solve_factored", lambda d, meq, a: lib.qpb_solve_factored(ctypes.byref(d), meq, *a, None)),
             ("qpb_solve_factored_host", lambda d, meq, a: lib.qpb_solve_factored_host(ctypes.byref(d), meq, *a)))
    for name, call in calls:
        # the descriptor's own rules come first, as in qpb_solve
        assert call(Desc(0, 0, 4, 0, 0, 0.0), 0, null) == INVALID, name
        assert call(Desc(129, 32, 4, 0, 0, 0.0), 0, null) == UNSUPPORTED, name
        assert call(Desc(16, 32, -1, 0, 0, 0.0), 0, null) == INVALID, name
        # then meq < 0, before the flags
        assert call(Desc(16, 32, 4, 0, FLAG_MIXED, 0.0), -1, ptrs) == INVALID and b"meq < 0" in err(), name
        # then the flags, also above the size limit
        for flags in (FLAG_DIAG_L2, FLAG_MIXED, FLAG_DIAG_WAVE, 4):
            for n, m in ((16, 32), (48, 96)):
                assert call(Desc(n, m, 4, 0, flags, 0.0), 0, ptrs) == INVALID, (name, flags, n, m)
                assert b"flags" in err()
        # then the size, before meq > m, batch == 0 and the pointers
        for n, m in ((33, 1), (33, 0), (32, 65), (16, 65), (33, 40), (128, 256)):
            for meq, batch, args in ((0, 4, ptrs), (0, 0, null), (m + 1, 4, null)):
                assert call(Desc(n, m, batch, 0, 0, 0.0), meq, args) == UNSUPPORTED, (name, n, m)
                assert b"factored kernels" in err() and b"n<=32" in err() and b"m<=64" in err()
        # then meq > m, before batch == 0
        for n, m in ((16, 32), (20, 40), (5, 0)):
            for batch, args in ((4, ptrs), (0, null)):
                assert call(Desc(n, m, batch, 0, 0, 0.0), m + 1, args) == INVALID, (name, n, m)
                assert b"meq=" in err()
        # batch 0 is a no-op before the pointers are looked at
        for n, m, meq in ((16, 32, 4), (20, 40, 0), (32, 64, 64), (3, 0, 0)):
            assert call(Desc(n, m, 0, 0, 0, 0.0), meq, null) == 0, (name, n, m)
        # missing pointers: fac, f, x and status always (iters may be NULL) ...
        for n, m in ((16, 32), (20, 33), (3, 0)):
            for k in (SF_, SFF_, SX_, SST_):
                args = list(ptrs)
                args[k] = None
                assert call(Desc(n, m, 4, 0, 0, 0.0), 0, args) == INVALID and b"required" in err(), (name, n, m, k)
        # ... b, lam and active when m > 0 only
        for k in (SB_, SLAM_, SACT_):
            args = list(ptrs)
            args[k] = None
            assert call(Desc(16, 32, 4, 0, 0, 0.0), 2, args) == INVALID, (name, k)
            assert call(Desc(20, 33, 4, 0, 0, 0.0), 0, args) == INVALID, (name, k)
    if not _device_present():
        # a valid call with no device fails loudly last
        for n, m, meq in ((16, 32, 0), (16, 32, 4), (20, 40, 3), (32, 64, 0)):
            args = list(ptrs)
            args[SIT_] = None
            d = Desc(n, m, 4, 0, 0, 0.0)
            assert lib.qpb_solve_factored(ctypes.byref(d), meq, *args, None) == NO_DEVICE, (n, m)
            assert b"no HIP device" in err()
            assert lib.qpb_solve_factored_host(ctypes.byref(d), meq, *args) == NO_DEVICE, (n, m)
        args = list(ptrs)
        args[SB_] = args[SLAM_] = args[SACT_] = None
        assert lib.qpb_solve_factored(ctypes.byref(Desc(3, 0, 4, 0, 0, 0.0)), 0, *args, None) == NO_DEVICE


def test_version_names_the_factored_kernels_beside_the_old_ones():
    lib = _lib()
    lib.qpb_version.restype = ctypes.c_char_p
    v = lib.qpb_version().decode()
    assert v.startswith("qpb 0.14 ")
    assert "gi_fact v1.0" in v
    tokens = [t.strip() for t in v[v.index("(") + 1:].split(";")]
    assert any(t.startswith("gi_fact v1.0:") for t in tokens)
    for old in ("gfx950", "gi_dense v11.7", "gi_box v2.2", "gi_wave v6.7", "gi_gram v4.5", "ref v6", "gi_eq v1.0",
                "kkt_bwd v1.1", "kkt_bwd_box v1.0", "gi_shared v1.0", "kkt_bwd_sum v1.0", "gi_range v1.0"):
        assert any(t.startswith(old) for t in tokens), old


def test_python_binding_has_the_calls():
    if os.environ.get("QPB_SANITIZED"):
        return  # imports torch
    import qpb
    for name in ("factor_shared", "factor_shared_host", "solve_factored", "solve_factored_host", "factor_doubles"):
        assert callable(getattr(qpb, name)), name
    assert qpb.SharedFactor._fields == ("fac", "n", "m", "status")
    assert qpb.factor_doubles(16, 32) == _lib().qpb_factor_doubles(16, 32)
    import inspect

    import qpb.diff
    assert inspect.signature(qpb.diff.solve).parameters["prefactor"].default is False
