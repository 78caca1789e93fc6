"""CPU tests of the boundary of qpb_solve_range_box (in the style of
test_abi_range.py): the two entry points are exported, the launchers stay
hidden, and every argument error is returned before any device work, each with
its code, in qpb.h's order.  desc->m is mg, the number of general rows."""
import ctypes
import os
import subprocess

from conftest import ROOT

LIB = os.environ.get("QPB_LIB", os.path.join(ROOT, "embedded-qp-solver_amd", "lib", "libqpb.so"))
INVALID, UNSUPPORTED, NO_DEVICE = -1, -2, -4
FLAG_DIAG_L2, FLAG_MIXED, FLAG_DIAG_WAVE = 1, 32, 256
# H, f, G, bl, bu, lb, ub, x, lam, active, lower, status, iters
H_, F_, G_, BL_, BU_, LB_, UB_, X_, LAM_, ACT_, LOW_, ST_, IT_ = range(13)


class Desc(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("m", ctypes.c_int32), ("batch", ctypes.c_int64),
                ("max_iter", ctypes.c_int32), ("flags", ctypes.c_int32), ("feas_tol", ctypes.c_double)]


def _lib():
    lib = ctypes.CDLL(LIB)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.qpb_last_error.restype = ctypes.c_char_p
    lib.qpb_solve_range_box.argtypes = [ctypes.POINTER(Desc), i32, i32] + [vp] * 14
    lib.qpb_solve_range_box_host.argtypes = [ctypes.POINTER(Desc), i32, i32] + [vp] * 13
    return lib


def _device_present():
    if os.environ.get("QPB_SANITIZED"):
        return False
    import torch
    return torch.cuda.is_available()


def test_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {"qpb_solve_range_box", "qpb_solve_range_box_host"} <= syms
    assert not {s for s in syms if s.startswith("qpb_launch_")}


def _calls(lib):
    return (("qpb_solve_range_box",
             lambda d, meq, sh, a: lib.qpb_solve_range_box(ctypes.byref(d), meq, sh, *a, None)),
            ("qpb_solve_range_box_host",
             lambda d, meq, sh, a: lib.qpb_solve_range_box_host(ctypes.byref(d), meq, sh, *a)))


def test_argument_errors_without_gpu():
    lib = _lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    null, ptrs = [None] * 13, [p] * 13
    err = lib.qpb_last_error
    for name, call in _calls(lib):
        for sh in (0, 1, 2, 3):
            # 1. the descriptor's own rules come first, as in qpb_solve, with m = mg
            assert call(Desc(0, 0, 4, 0, 0, 0.0), 0, sh, null) == INVALID, name
            assert call(Desc(16, -1, 4, 0, 0, 0.0), 0, sh, null) == INVALID, name
            assert call(Desc(129, 32, 4, 0, 0, 0.0), 0, sh, null) == UNSUPPORTED, name
            assert b"range_box" not in err()  # the descriptor's message, not this call's
            assert call(Desc(16, 16, -1, 0, 0, 0.0), 0, sh, null) == INVALID, name
            # 2. then meq < 0, before the flags
            assert call(Desc(16, 16, 4, 0, FLAG_MIXED, 0.0), -1, sh, ptrs) == INVALID and b"meq < 0" in err(), name
            # ... the flags, also above the size limit and with a bad `shared`
            for flags in (FLAG_DIAG_L2, FLAG_MIXED, FLAG_DIAG_WAVE, 4):
                for n, mg in ((16, 16), (48, 96)):
                    assert call(Desc(n, mg, 4, 0, flags, 0.0), 0, sh | 4, ptrs) == INVALID, (name, flags, n, mg)
                    assert b"flags" in err()
        # ... the bits of `shared`, before the size, meq > mg and batch == 0
        for sh in (4, 7, 8, -1, 1 << 30):
            for n, mg, meq, batch in ((16, 16, 0, 4), (48, 96, 0, 4), (16, 16, 17, 4), (16, 16, 0, 0)):
                assert call(Desc(n, mg, batch, 0, 0, 0.0), meq, sh, null) == INVALID, (name, sh, n, mg)
                assert b"QPB_SHARED_H" in err()
        # 3. then the size, whatever is shared: n <= 32 and mg + n <= 64, a message that names the
        # call and the limit, before meq > mg, batch == 0 and the pointers
        for sh in (0, 1, 2, 3):
            for n, mg in ((33, 0), (32, 33), (33, 1), (1, 64), (16, 49), (20, 45), (128, 128), (64, 0)):
                for meq, batch, args in ((0, 4, ptrs), (0, 0, null), (mg + 1, 4, null)):
                    assert call(Desc(n, mg, batch, 0, 0, 0.0), meq, sh, args) == UNSUPPORTED, (name, n, mg, sh)
                    assert b"range_box" in err() and b"n<=32" in err() and b"mg+n<=64" in err()
        # 4. then meq > mg
        for sh in (0, 1, 2, 3):
            for n, mg in ((16, 16), (20, 40), (5, 0), (32, 32)):
                for batch, args in ((4, ptrs), (0, null)):
                    assert call(Desc(n, mg, batch, 0, 0, 0.0), mg + 1, sh, args) == INVALID, (name, n, mg, sh)
                    assert b"meq=" in err()
        # 5. batch 0 is a no-op before the pointers are looked at
        for sh in (0, 1, 2, 3):
            for n, mg, meq in ((16, 16, 4), (20, 40, 0), (32, 32, 32), (3, 0, 0), (1, 63, 0)):
                assert call(Desc(n, mg, 0, 0, 0, 0.0), meq, sh, null) == 0, (name, n, mg, sh)
        # 6. missing pointers: H, f, x, lam, active and status always (lower and iters may be NULL) ...
        for sh in (0, 1, 2, 3):
            for n, mg in ((16, 16), (20, 33), (3, 0)):
                for k in (H_, F_, X_, LAM_, ACT_, ST_):
                    args = list(ptrs)
                    args[k] = None
                    assert call(Desc(n, mg, 4, 0, 0, 0.0), 0, sh, args) == INVALID, (name, n, mg, k)
                    assert b"required" in err()
            # ... G when mg > 0
            args = list(ptrs)
            args[G_] = None
            for n, mg in ((16, 16), (20, 33), (1, 1)):
                assert call(Desc(n, mg, 4, 0, 0, 0.0), 0, sh, args) == INVALID, (name, n, mg)
                assert b"G is required" in err()
            # ... and at least one of the four bounds
            args = list(ptrs)
            args[BL_] = args[BU_] = args[LB_] = args[UB_] = None
            for n, mg in ((16, 16), (20, 33), (3, 0)):
                assert call(Desc(n, mg, 4, 0, 0, 0.0), 0, sh, args) == INVALID, (name, n, mg)
                assert b"at least one of bl, bu, lb and ub" in err()
    if not _device_present():
        # 7. a valid call with no device fails loudly last: any one bound alone, lower and iters NULL
        bounds = (BL_, BU_, LB_, UB_)
        for sh in (0, 1, 2, 3):
            for n, mg, meq in ((16, 16, 0), (16, 16, 4), (20, 40, 3), (32, 32, 0), (1, 1, 1), (12, 20, 0)):
                for drop in ((), (LOW_, IT_)) + tuple(tuple(b for b in bounds if b != keep) for keep in bounds):
                    args = list(ptrs)
                    for k in drop:
                        args[k] = None
                    d = Desc(n, mg, 4, 0, 0, 0.0)
                    assert lib.qpb_solve_range_box(ctypes.byref(d), meq, sh, *args, None) == NO_DEVICE, (n, mg, sh, drop)
                    assert b"no HIP device" in err()
                    assert lib.qpb_solve_range_box_host(ctypes.byref(d), meq, sh, *args) == NO_DEVICE, (n, mg, sh, drop)
        # mg == 0: G may be NULL, and the rows' bounds with it
        args = list(ptrs)
        args[G_] = args[BL_] = args[BU_] = None
        for n in (1, 16, 17, 32):
            assert lib.qpb_solve_range_box(ctypes.byref(Desc(n, 0, 4, 0, 0, 0.0)), 0, 3, *args, None) == NO_DEVICE
            assert lib.qpb_solve_range_box_host(ctypes.byref(Desc(n, 0, 4, 0, 0, 0.0)), 0, 0, *args) == NO_DEVICE


def test_version_names_the_range_box_forms_beside_the_old_ones():
    lib = _lib()
    lib.qpb_version.restype = ctypes.c_char_p
    v = lib.qpb_version().decode()
    assert v.startswith("qpb 0.14 ")
    tokens = [t.strip() for t in v[v.index("(") + 1:].split(";")]
    assert any(t.startswith("gi_range_box v1.0:") for t in tokens)
    for old in ("gfx950", "gi_dense v11.7", "gi_box v2.2", "gi_wave v6.7", "gi_gram v4.5", "ref v6", "gi_eq v1.0",
                "kkt_bwd v1.1", "kkt_bwd_box v1.0", "gi_shared v1.0", "kkt_bwd_sum v1.0", "gi_range v1.0:",
                "gi_fact v1.0", "gi_rfact v1.0", "box_shared v1.0", "box_fact v1.0"):
        assert any(t.startswith(old) for t in tokens), old


def test_python_binding_has_the_calls():
    if os.environ.get("QPB_SANITIZED"):
        return  # imports torch
    import qpb
    for name in ("solve_range_box", "solve_range_box_host", "solve_range"):
        assert callable(getattr(qpb, name)), name
    assert qpb.RangeSolution._fields == ("x", "lam", "active", "lower", "status", "iters")
    assert qpb._lib.qpb_solve_range_box.argtypes is not None and len(qpb._lib.qpb_solve_range_box.argtypes) == 17
    import qpb.diff
    assert callable(qpb.diff.solve_range_box) and callable(qpb.diff.solve_range)
