"""CPU tests of the boundary of qpb_factor_box and qpb_solve_box_factored (in the
style of test_abi_box_shared.py and test_abi_factored.py): the five entry
points are exported, the launchers stay hidden, the buffer's size is the
layout's (csrc/qpb_factor.h, bxfct), and every argument error is returned before
any device work, each with its code, in qpb.h's order."""
import ctypes
import os
import subprocess

from conftest import ROOT

LIB = os.environ.get("QPB_LIB", os.path.join(ROOT, "embedded-qp-solver_amd", "lib", "libqpb.so"))
INVALID, UNSUPPORTED, NO_DEVICE = -1, -2, -4
FLAG_DIAG_L2, FLAG_MIXED, FLAG_DIAG_WAVE = 1, 32, 256
# the solve: bxfac, f, lb, ub, x, lam, active, status, iters
FAC_, FF_, FLB_, FUB_, FX_, FLAM_, FACT_, FST_, FIT_ = range(9)
# bxfct::layout(n).size: header 8, L, the rows of L^-T, their squared norms
SIZE16, SIZE32 = 8 + 256 + 256 + 16, 8 + 528 + 1024 + 32
NAMES = ("qpb_factor_box_doubles", "qpb_factor_box", "qpb_factor_box_host", "qpb_solve_box_factored",
         "qpb_solve_box_factored_host")


class Desc(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("m", ctypes.c_int32), ("batch", ctypes.c_int64),
                ("max_iter", ctypes.c_int32), ("flags", ctypes.c_int32), ("feas_tol", ctypes.c_double)]


def _lib():
    lib = ctypes.CDLL(LIB)
    vp = ctypes.c_void_p
    lib.qpb_last_error.restype = ctypes.c_char_p
    lib.qpb_factor_box_doubles.argtypes = [ctypes.c_int32]
    lib.qpb_factor_box_doubles.restype = ctypes.c_int64
    lib.qpb_factor_box.argtypes = [ctypes.c_int32] + [vp] * 4
    lib.qpb_factor_box_host.argtypes = [ctypes.c_int32] + [vp] * 3
    lib.qpb_solve_box_factored.argtypes = [ctypes.POINTER(Desc)] + [vp] * 10
    lib.qpb_solve_box_factored_host.argtypes = [ctypes.POINTER(Desc)] + [vp] * 9
    return lib


def _device_present():
    if os.environ.get("QPB_SANITIZED"):
        return False
    import torch
    return torch.cuda.is_available()


def _aligned(buf, off=0):
    """A pointer into `buf` at a 16-byte boundary plus `off` bytes."""
    a = ctypes.addressof(buf)
    return ctypes.c_void_p(a + (-a % 16) + off)


def test_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(NAMES) <= syms
    assert not {s for s in syms if s.startswith("qpb_launch_")}


def test_factor_box_doubles():
    lib = _lib()
    assert lib.qpb_factor_box_doubles(1) == SIZE16
    assert lib.qpb_factor_box_doubles(16) == SIZE16
    assert lib.qpb_factor_box_doubles(17) == SIZE32
    assert lib.qpb_factor_box_doubles(32) == SIZE32
    assert lib.qpb_factor_box_doubles(0) == INVALID
    assert lib.qpb_factor_box_doubles(-3) == INVALID
    assert lib.qpb_factor_box_doubles(33) == UNSUPPORTED
    assert b"n<=32" in lib.qpb_last_error()
    assert lib.qpb_factor_box_doubles(128) == UNSUPPORTED


def _factor_calls(lib):
    return (("qpb_factor_box", lambda n, a: lib.qpb_factor_box(n, *a, None), True),
            ("qpb_factor_box_host", lambda n, a: lib.qpb_factor_box_host(n, *a), False))


def test_factor_argument_errors_without_gpu():
    lib = _lib()
    buf = ctypes.create_string_buffer(128)
    p, odd = _aligned(buf), _aligned(buf, 8)
    for name, call, device_ptrs in _factor_calls(lib):
        # 1. n, before the pointers
        for n in (0, -1):
            assert call(n, [None, None, None]) == INVALID, (name, n)
        for n in (33, 64, 128, 129):
            assert call(n, [None, None, None]) == UNSUPPORTED, (name, n)
            assert b"n<=32" in lib.qpb_last_error()
            assert call(n, [p, odd, p]) == UNSUPPORTED, (name, n)
        # 2. H and bxfac are required, fstatus is not
        for n in (1, 16, 17, 32):
            assert call(n, [None, p, p]) == INVALID, (name, n)
            assert b"required" in lib.qpb_last_error()
            assert call(n, [p, None, p]) == INVALID, (name, n)
            assert b"required" in lib.qpb_last_error()
            # 3. the device call's bxfac on a 16-byte boundary, after the missing pointers
            if device_ptrs:
                assert call(n, [None, odd, p]) == INVALID and b"required" in lib.qpb_last_error()
                assert call(n, [p, odd, p]) == INVALID, (name, n)
                assert b"aligned" in lib.qpb_last_error()
                assert call(n, [p, odd, None]) == INVALID and b"aligned" in lib.qpb_last_error()
    if not _device_present():
        # 4. a valid call with no device fails loudly last, with or without fstatus
        for name, call, _ in _factor_calls(lib):
            for n in (1, 16, 17, 32):
                for fst in (p, None):
                    assert call(n, [p, p, fst]) == NO_DEVICE, (name, n)
                    assert b"no HIP device" in lib.qpb_last_error()


def _solve_calls(lib):
    return (("qpb_solve_box_factored", lambda d, a: lib.qpb_solve_box_factored(ctypes.byref(d), *a, None), True),
            ("qpb_solve_box_factored_host", lambda d, a: lib.qpb_solve_box_factored_host(ctypes.byref(d), *a), False))


def test_solve_argument_errors_without_gpu():
    lib = _lib()
    buf = ctypes.create_string_buffer(128)
    p, odd = _aligned(buf), _aligned(buf, 8)
    null, ptrs = [None] * 9, [p] * 9
    for name, call, device_ptrs in _solve_calls(lib):
        # 1. the descriptor as qpb_solve_box ...
        assert call(Desc(0, 0, 4, 0, 0, 0.0), null) == INVALID, name
        assert call(Desc(129, 258, 4, 0, 0, 0.0), null) == UNSUPPORTED, name
        assert b"n<=32" not in lib.qpb_last_error()  # the build's limit, not this call's
        assert call(Desc(16, 32, -1, 0, 0, 0.0), null) == INVALID, name
        # ... then m == 2n, before the flags, the size and batch == 0
        for n, m, flags, batch in ((16, 31, 0, 4), (16, 0, 0, 4), (16, 33, FLAG_MIXED, 4), (48, 95, 0, 4),
                                   (5, 9, 0, 0), (33, 64, 4, 0), (128, 255, 0, 0)):
            assert call(Desc(n, m, batch, 0, flags, 0.0), null) == INVALID, (name, n, m)
            assert b"2n" in lib.qpb_last_error() and b"flags" not in lib.qpb_last_error()
        # 2. the flags must be 0, also above the size limit and with an empty batch
        for flags in (FLAG_DIAG_L2, FLAG_MIXED, FLAG_DIAG_WAVE, 4):
            for n in (16, 20, 48):
                for batch, args in ((4, ptrs), (0, null)):
                    assert call(Desc(n, 2 * n, batch, 0, flags, 0.0), args) == INVALID, (name, flags, n)
                    assert b"flags" in lib.qpb_last_error()
        # 3. the size: n > 32 is unsupported, before batch == 0 and the pointers
        for n in (33, 40, 64, 128):
            for batch, args in ((4, ptrs), (0, null), (4, null)):
                assert call(Desc(n, 2 * n, batch, 0, 0, 0.0), args) == UNSUPPORTED, (name, n, batch)
                assert b"n<=32" in lib.qpb_last_error() and b"qpb_solve_box_factored" in lib.qpb_last_error()
        # 4. batch 0 is a no-op before the pointers are looked at, a misaligned buffer included
        for n in (1, 16, 17, 32):
            assert call(Desc(n, 2 * n, 0, 0, 0, 0.0), null) == 0, (name, n)
            assert call(Desc(n, 2 * n, 0, 0, 0, 0.0), [odd] * 9) == 0, (name, n)
        # 5. missing pointers: bxfac, f, x, lam, active and status
        for n in (1, 16, 20, 32):
            for k in (FAC_, FF_, FX_, FLAM_, FACT_, FST_):
                args = list(ptrs)
                args[k] = None
                assert call(Desc(n, 2 * n, 4, 0, 0, 0.0), args) == INVALID, (name, n, k)
                assert b"required" in lib.qpb_last_error()
                if device_ptrs and k != FAC_:  # ... before the alignment
                    args[FAC_] = odd
                    assert call(Desc(n, 2 * n, 4, 0, 0, 0.0), args) == INVALID, (name, n, k)
                    assert b"required" in lib.qpb_last_error()
            # 6. the device call's bxfac on a 16-byte boundary; lb, ub and iters may be NULL
            if device_ptrs:
                for drop in ((), (FLB_, FUB_, FIT_)):
                    args = [None if k in drop else p for k in range(9)]
                    args[FAC_] = odd
                    assert call(Desc(n, 2 * n, 4, 0, 0, 0.0), args) == INVALID, (name, n, drop)
                    assert b"aligned" in lib.qpb_last_error()
    if not _device_present():
        # 7. a valid call with no device fails loudly last: lb, ub and iters may be NULL
        for n in (1, 16, 20, 32):
            d = Desc(n, 2 * n, 4, 0, 0, 0.0)
            for drop in ((), (FLB_,), (FUB_,), (FLB_, FUB_, FIT_)):
                args = [None if k in drop else p for k in range(9)]
                for name, call, _ in _solve_calls(lib):
                    assert call(d, args) == NO_DEVICE, (name, n, drop)
                    assert b"no HIP device" in lib.qpb_last_error()


def test_unsupported_before_the_empty_batch():
    """n = 33 and n = 128: UNSUPPORTED before batch == 0 is looked at, and m != 2n INVALID before that."""
    lib = _lib()
    null = [None] * 9
    for name, call, _ in _solve_calls(lib):
        for n in (33, 128):
            assert call(Desc(n, 2 * n, 0, 0, 0, 0.0), null) == UNSUPPORTED, (name, n)
            assert call(Desc(n, 2 * n, 4, 0, 0, 0.0), null) == UNSUPPORTED, (name, n)
            assert call(Desc(n, 2 * n - 1, 0, 0, 0, 0.0), null) == INVALID, (name, n)
            assert b"2n" in lib.qpb_last_error()
        assert call(Desc(129, 258, 0, 0, 0, 0.0), null) == UNSUPPORTED, name


def test_version_keeps_its_tokens_and_names_the_form():
    lib = _lib()
    lib.qpb_version.restype = ctypes.c_char_p
    v = lib.qpb_version().decode()
    assert v.startswith("qpb 0.14 ")
    inner = v.split("(", 1)[1].rsplit(")", 1)[0]
    heads = {part.split(":", 1)[0].strip() for part in inner.split(";") if ":" in part}
    assert {"box_fact v1.0", "box_shared v1.0", "gi_fact v1.0", "gi_box v2.2", "kkt_bwd_box v1.0"} <= heads


def test_python_binding_has_the_calls():
    if os.environ.get("QPB_SANITIZED"):
        return  # imports torch
    import qpb
    for name in ("factor_box_doubles", "factor_box", "factor_box_host", "solve_box_factored",
                 "solve_box_factored_host", "BoxFactor"):
        assert callable(getattr(qpb, name)), name
    assert qpb.factor_box_doubles(16) == SIZE16 and qpb.factor_box_doubles(17) == SIZE32
    assert qpb.BoxFactor._fields == ("fac", "n", "status")
