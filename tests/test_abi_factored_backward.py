"""CPU tests of the boundary of qpb_factor_backward_doubles,
qpb_factor_shared_backward and qpb_solve_factored_backward (in the style of
test_abi_factored.py): the five entry points are exported, the launchers stay
hidden, the size of a backward buffer is host arithmetic, and every argument
error is returned before any device work, each with its code, in qpb.h's order."""
import ctypes
import os
import subprocess

from conftest import ROOT

LIB = os.environ.get("QPB_LIB", os.path.join(ROOT, "embedded-qp-solver_amd", "lib", "libqpb.so"))
INVALID, UNSUPPORTED, NO_DEVICE = -1, -2, -4
FLAG_DIAG_L2, FLAG_MIXED, FLAG_DIAG_WAVE = 1, 32, 256
# solve: bfac, x, lam, active, status, gx, gH, gf, gA, gb
SF_, SX_, SLAM_, SACT_, SST_, SGX_, SGH_, SGF_, SGA_, SGB_ = range(10)
# factor: H, A, bfac, fstatus
FH_, FA_, FF_, FS_ = range(4)
HDR = 8


def layout_doubles(n, m):
    """csrc/qpb_factor.h, bfct::layout(n, m).size: the header, then per class
    L | 1 / L_kk | (the multipliers) | D."""
    if n <= 16 and m <= 32:
        return HDR + 160 + 16 + 256 + 256 * (1 if m <= 16 else 2)
    return HDR + 32 * 33 + 32 + 32 * m


class Desc(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("m", ctypes.c_int32), ("batch", ctypes.c_int64),
                ("max_iter", ctypes.c_int32), ("flags", ctypes.c_int32), ("feas_tol", ctypes.c_double)]


def _lib():
    lib = ctypes.CDLL(LIB)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.qpb_last_error.restype = ctypes.c_char_p
    lib.qpb_factor_backward_doubles.argtypes = [i32, i32]
    lib.qpb_factor_backward_doubles.restype = ctypes.c_int64
    lib.qpb_factor_shared_backward.argtypes = [i32, i32] + [vp] * 5
    lib.qpb_factor_shared_backward_host.argtypes = [i32, i32] + [vp] * 4
    lib.qpb_solve_factored_backward.argtypes = [ctypes.POINTER(Desc)] + [vp] * 11
    lib.qpb_solve_factored_backward_host.argtypes = [ctypes.POINTER(Desc)] + [vp] * 10
    return lib


def _device_present():
    if os.environ.get("QPB_SANITIZED"):
        return False
    import torch
    return torch.cuda.is_available()


def _aligned16(buf, off=0):
    """A pointer into `buf`, `off` bytes past a 16-byte boundary (bfac must be on one)."""
    a = ctypes.addressof(buf)
    return ctypes.c_void_p(((a + 15) & ~15) + off)


def test_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {"qpb_factor_backward_doubles", "qpb_factor_shared_backward", "qpb_factor_shared_backward_host",
            "qpb_solve_factored_backward", "qpb_solve_factored_backward_host"} <= syms
    assert not {s for s in syms if s.startswith("qpb_launch_")}


def test_factor_backward_doubles():
    lib = _lib()
    err = lib.qpb_last_error
    assert lib.qpb_factor_backward_doubles(1, 0) == 8 + 160 + 16 + 256 + 256
    assert lib.qpb_factor_backward_doubles(16, 32) == 8 + 160 + 16 + 256 + 512
    assert lib.qpb_factor_backward_doubles(16, 33) == 8 + 1056 + 32 + 33 * 32
    assert lib.qpb_factor_backward_doubles(17, 0) == 8 + 1056 + 32
    assert lib.qpb_factor_backward_doubles(32, 64) == 8 + 1056 + 32 + 2048
    for n in (1, 5, 16, 17, 32):
        for m in range(0, 65):
            k = lib.qpb_factor_backward_doubles(n, m)
            assert k == layout_doubles(n, m), (n, m, k)
            # room for L and D at least, and a whole number of 16-byte pieces
            assert k >= n * (n + 1) // 2 + m * n and k % 2 == 0, (n, m, k)
    assert lib.qpb_factor_backward_doubles(33, 0) == UNSUPPORTED and b"n<=32" in err() and b"m<=64" in err()
    assert lib.qpb_factor_backward_doubles(16, 65) == UNSUPPORTED
    assert lib.qpb_factor_backward_doubles(0, 0) == INVALID
    assert lib.qpb_factor_backward_doubles(1, -1) == INVALID
    assert lib.qpb_factor_backward_doubles(0, 65) == INVALID  # the shape's own rules before the size


def test_factor_argument_errors_without_gpu():
    lib = _lib()
    buf = ctypes.create_string_buffer(96)
    p = _aligned16(buf)
    null, ptrs = [None] * 4, [p] * 4
    err = lib.qpb_last_error
    calls = (("qpb_factor_shared_backward", lambda n, m, a: lib.qpb_factor_shared_backward(n, m, *a, None)),
             ("qpb_factor_shared_backward_host", lambda n, m, a: lib.qpb_factor_shared_backward_host(n, m, *a)))
    for name, call in calls:
        # the shape first, as a descriptor's
        assert call(0, 0, null) == INVALID, name
        assert call(16, -1, ptrs) == INVALID, name
        assert call(0, 65, ptrs) == INVALID, name
        # then the size, before the pointers
        for n, m in ((33, 0), (33, 1), (16, 65), (32, 65), (128, 256)):
            for args in (null, ptrs):
                assert call(n, m, args) == UNSUPPORTED, (name, n, m)
                assert b"factored backward kernels" in err() and b"n<=32" in err() and b"m<=64" in err()
        # then the pointers: H and bfac always (fstatus may be NULL), A when m > 0 only
        for n, m in ((16, 32), (20, 40), (3, 0)):
            for k in (FH_, FF_):
                args = list(ptrs)
                args[k] = None
                assert call(n, m, args) == INVALID and b"required" in err(), (name, n, m, k)
        args = list(ptrs)
        args[FA_] = None
        assert call(16, 32, args) == INVALID and b"A is required" in err(), name
        assert call(20, 33, args) == INVALID, name
    # then the alignment of the device buffer, after the pointers and before the device
    for n, m in ((16, 32), (20, 40), (3, 0)):
        args = list(ptrs)
        args[FF_] = _aligned16(buf, 8)
        assert lib.qpb_factor_shared_backward(n, m, *args, None) == INVALID and b"16-byte" in err(), (n, m)
        args[FH_] = None
        assert lib.qpb_factor_shared_backward(n, m, *args, None) == INVALID and b"required" in err(), (n, m)
    if not _device_present():
        # a valid call with no device fails loudly last: fstatus NULL, A NULL at m == 0
        for n, m in ((16, 32), (5, 9), (20, 40), (32, 64)):
            args = list(ptrs)
            args[FS_] = None
            assert lib.qpb_factor_shared_backward(n, m, *args, None) == NO_DEVICE, (n, m)
            assert b"no HIP device" in err()
            assert lib.qpb_factor_shared_backward_host(n, m, *args) == NO_DEVICE, (n, m)
        assert lib.qpb_factor_shared_backward(3, 0, p, None, p, None, None) == NO_DEVICE


def test_solve_argument_errors_without_gpu():
    lib = _lib()
    buf = ctypes.create_string_buffer(96)
    p = _aligned16(buf)
    null, ptrs = [None] * 10, [p] * 10
    err = lib.qpb_last_error
    calls = (("qpb_solve_factored_backward", lambda d, a: lib.qpb_solve_factored_backward(ctypes.byref(d), *a, None)),
             ("qpb_solve_factored_backward_host",
              lambda d, a: lib.qpb_solve_factored_backward_host(ctypes.byref(d), *a)))
    for name, call in calls:
        # the descriptor's own rules come first, as in qpb_solve
        assert call(Desc(0, 0, 4, 0, 0, 0.0), null) == INVALID, name
        assert call(Desc(129, 32, 4, 0, 0, 0.0), null) == UNSUPPORTED, name
        assert call(Desc(16, 32, -1, 0, 0, 0.0), null) == INVALID, name
        # then the flags, also above the size limit
        for flags in (FLAG_DIAG_L2, FLAG_MIXED, FLAG_DIAG_WAVE, 4):
            for n, m in ((16, 32), (48, 96)):
                assert call(Desc(n, m, 4, 0, flags, 0.0), ptrs) == INVALID, (name, flags, n, m)
                assert b"flags" in err()
        # then the size, before batch == 0 and the pointers
        for n, m in ((33, 1), (33, 0), (32, 65), (16, 65), (33, 40), (128, 256)):
            for batch, args in ((4, ptrs), (0, null), (4, null)):
                assert call(Desc(n, m, batch, 0, 0, 0.0), args) == UNSUPPORTED, (name, n, m)
                assert b"factored backward kernels" in err() and b"n<=32" in err() and b"m<=64" in err()
        # batch 0 is a no-op before the pointers are looked at
        for n, m in ((16, 32), (20, 40), (32, 64), (3, 0)):
            assert call(Desc(n, m, 0, 0, 0, 0.0), null) == 0, (name, n, m)
        # missing pointers: bfac, x and gx always (status may be NULL) ...
        for n, m in ((16, 32), (20, 33), (3, 0)):
            for k in (SF_, SX_, SGX_):
                args = list(ptrs)
                args[k] = None
                assert call(Desc(n, m, 4, 0, 0, 0.0), args) == INVALID and b"required" in err(), (name, n, m, k)
            args = list(ptrs)
            args[SST_] = None
            if not _device_present():
                assert call(Desc(n, m, 4, 0, 0, 0.0), args) == NO_DEVICE, (name, n, m)
        # ... lam and active when m > 0 only
        for k in (SLAM_, SACT_):
            args = list(ptrs)
            args[k] = None
            assert call(Desc(16, 32, 4, 0, 0, 0.0), args) == INVALID and b"lam and active" in err(), (name, k)
            assert call(Desc(20, 33, 4, 0, 0, 0.0), args) == INVALID, (name, k)
        # ... and at least one output; with m == 0 gA and gb are not outputs
        args = list(ptrs)
        args[SGH_] = args[SGF_] = args[SGA_] = args[SGB_] = None
        assert call(Desc(16, 32, 4, 0, 0, 0.0), args) == INVALID and b"at least one" in err(), name
        args[SGA_] = args[SGB_] = p
        assert call(Desc(3, 0, 4, 0, 0, 0.0), args) == INVALID and b"at least one" in err(), name
    # then the alignment of the device buffer, after the pointers and before the device
    for n, m in ((16, 32), (20, 40), (3, 0)):
        args = list(ptrs)
        args[SF_] = _aligned16(buf, 8)
        d = Desc(n, m, 4, 0, 0, 0.0)
        assert lib.qpb_solve_factored_backward(ctypes.byref(d), *args, None) == INVALID and b"16-byte" in err()
        args[SX_] = None
        assert lib.qpb_solve_factored_backward(ctypes.byref(d), *args, None) == INVALID and b"required" in err()
    if not _device_present():
        # a valid call with no device fails loudly last, with any one output
        for n, m in ((16, 32), (5, 9), (20, 40), (32, 64)):
            d = Desc(n, m, 4, 0, 0, 0.0)
            for keep in (SGH_, SGF_, SGA_, SGB_):
                args = list(ptrs)
                for k in (SGH_, SGF_, SGA_, SGB_):
                    args[k] = p if k == keep else None
                assert lib.qpb_solve_factored_backward(ctypes.byref(d), *args, None) == NO_DEVICE, (n, m, keep)
                assert b"no HIP device" in err()
                assert lib.qpb_solve_factored_backward_host(ctypes.byref(d), *args) == NO_DEVICE, (n, m, keep)
        args = list(ptrs)
        args[SLAM_] = args[SACT_] = args[SGA_] = args[SGB_] = None
        assert lib.qpb_solve_factored_backward(ctypes.byref(Desc(3, 0, 4, 0, 0, 0.0)), *args, None) == NO_DEVICE


def test_version_names_the_factored_backward_beside_the_old_ones():
    lib = _lib()
    lib.qpb_version.restype = ctypes.c_char_p
    v = lib.qpb_version().decode()
    assert v.startswith("qpb 0.14 ")
    tokens = [t.strip() for t in v[v.index("(") + 1:].split(";")]
    assert any(t.startswith("kkt_bwd_fact v1.0:") for t in tokens)
    for old in ("gfx950", "gi_dense v11.7", "gi_box v2.2", "gi_wave v6.7", "gi_gram v4.5", "ref v6", "gi_eq v1.0",
                "kkt_bwd v1.1", "kkt_bwd_box v1.0", "gi_shared v1.0", "kkt_bwd_sum v1.0", "gi_range v1.0",
                "gi_fact v1.0", "gi_rfact v1.0"):
        assert any(t.startswith(old) for t in tokens), old


def test_python_binding_has_the_calls():
    if os.environ.get("QPB_SANITIZED"):
        return  # imports torch
    import qpb
    for name in ("factor_shared_backward", "factor_shared_backward_host", "solve_factored_backward",
                 "solve_factored_backward_host", "factor_backward_doubles"):
        assert callable(getattr(qpb, name)), name
    assert qpb.BackwardFactor._fields == ("fac", "n", "m", "status")
    assert qpb.factor_backward_doubles(16, 32) == _lib().qpb_factor_backward_doubles(16, 32) == layout_doubles(16, 32)
    for n, m in ((33, 0), (16, 65)):
        try:
            qpb.factor_backward_doubles(n, m)
        except qpb.QPBError as e:
            assert e.code == qpb.ERR_UNSUPPORTED
        else:
            raise AssertionError((n, m))
