"""CPU tests of the boundary of qpb_solve_factored_backward_multi and
qpb_solve_box_backward_multi (in the style of test_abi_box_backward_dual.py and
test_abi_factored_backward_dual.py): the four entry points are exported, the
launchers stay hidden, and every argument error is returned before any device
work, each with its code, in qpb.h's order -- with glam given, NULL and odd
(never read: it is never required)."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT

LIB = os.environ.get("QPB_LIB", os.path.join(ROOT, "embedded-qp-solver_amd", "lib", "libqpb.so"))
INVALID, UNSUPPORTED, NO_DEVICE = -1, -2, -4
FLAG_DIAG_L2, FLAG_MIXED, FLAG_DIAG_WAVE = 1, 32, 256
SHARED_H, SHARED_A, SHARED_RHS, MAX_RHS = 1, 2, 4, 256
# factored: bfac, active, status | gx, glam, gf, gb
F_, FACT_, FST_, FGX_, FGM_, FGF_, FGB_ = range(7)
# box: H, active, status | gx, glam, gf, glb, gub
H_, ACT_, ST_, GX_, GM_, GF_, GL_, GU_ = range(8)
BOX_OUTPUTS = (GF_, GL_, GU_)
SYMBOLS = {"qpb_solve_factored_backward_multi", "qpb_solve_factored_backward_multi_host",
           "qpb_solve_box_backward_multi", "qpb_solve_box_backward_multi_host"}


class Desc(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("m", ctypes.c_int32), ("batch", ctypes.c_int64),
                ("max_iter", ctypes.c_int32), ("flags", ctypes.c_int32), ("feas_tol", ctypes.c_double)]


def _lib():
    lib = ctypes.CDLL(LIB)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.qpb_last_error.restype = ctypes.c_char_p
    lib.qpb_version.restype = ctypes.c_char_p
    lib.qpb_solve_factored_backward_multi.argtypes = [ctypes.POINTER(Desc)] + [vp] * 3 + [i32] * 2 + [vp] * 5
    lib.qpb_solve_factored_backward_multi_host.argtypes = [ctypes.POINTER(Desc)] + [vp] * 3 + [i32] * 2 + [vp] * 4
    lib.qpb_solve_box_backward_multi.argtypes = [ctypes.POINTER(Desc), i32] + [vp] * 3 + [i32] + [vp] * 6
    lib.qpb_solve_box_backward_multi_host.argtypes = [ctypes.POINTER(Desc), i32] + [vp] * 3 + [i32] + [vp] * 5
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


def test_symbols_and_version():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert SYMBOLS <= syms
    assert not {s for s in syms if s.startswith("qpb_launch_")}
    assert _lib().qpb_version().startswith(b"qpb 0.14")


def _factored_calls(lib):
    """Both entry points with the same (desc, nrhs, shared, seven array pointers)."""
    return (("qpb_solve_factored_backward_multi",
             lambda d, T, sh, a: lib.qpb_solve_factored_backward_multi(ctypes.byref(d), *a[:3], T, sh, *a[3:], None)),
            ("qpb_solve_factored_backward_multi_host",
             lambda d, T, sh, a: lib.qpb_solve_factored_backward_multi_host(ctypes.byref(d), *a[:3], T, sh, *a[3:])))


def _box_calls(lib):
    """Both entry points with the same (desc, shared, nrhs, eight array pointers)."""
    return (("qpb_solve_box_backward_multi",
             lambda d, sh, T, a: lib.qpb_solve_box_backward_multi(ctypes.byref(d), sh, *a[:3], T, *a[3:], None)),
            ("qpb_solve_box_backward_multi_host",
             lambda d, sh, T, a: lib.qpb_solve_box_backward_multi_host(ctypes.byref(d), sh, *a[:3], T, *a[3:])))


def test_factored_argument_errors_without_gpu():
    lib = _lib()
    err = lib.qpb_last_error
    buf = ctypes.create_string_buffer(96)
    p = _aligned16(buf)
    odd = _aligned16(buf, 1)  # misaligned: nothing is read before the checks are through
    null = [None] * 7
    for glam in (p, None, odd):
        ptrs = [p] * 7
        ptrs[FGM_] = glam
        for name, call in _factored_calls(lib):
            for shared in (0, SHARED_RHS):
                # 1. the descriptor, as qpb_solve checks it
                assert call(Desc(0, 0, 4, 0, 0, 0.0), 1, shared, null) == INVALID, name
                assert call(Desc(129, 32, 4, 0, 0, 0.0), 1, shared, null) == UNSUPPORTED, name
                assert b"n<=32" not in err()  # the build's limit, not this call's
                assert call(Desc(16, 32, -1, 0, 0, 0.0), 1, shared, null) == INVALID, name
                # 3. the flags: none selects anything here, also above the size limit and at batch == 0
                for flags in (FLAG_DIAG_L2, FLAG_MIXED, FLAG_DIAG_WAVE, 4):
                    for n, m in ((16, 32), (20, 40), (48, 16)):
                        for batch, args in ((4, ptrs), (0, null)):
                            assert call(Desc(n, m, batch, 0, flags, 0.0), 1, shared, args) == INVALID, (name, flags)
                            assert b"flags" in err() and b"backward_multi" in err()
                # ... nrhs, likewise, after the flags
                for T in (0, -1, MAX_RHS + 1):
                    for n, m, batch, args in ((16, 32, 4, ptrs), (48, 16, 4, ptrs), (16, 32, 0, null)):
                        assert call(Desc(n, m, batch, 0, 0, 0.0), T, shared, args) == INVALID, (name, T)
                        assert b"nrhs" in err() and b"256" in err()
                    assert call(Desc(16, 32, 4, 0, FLAG_MIXED, 0.0), T, shared, ptrs) == INVALID and b"flags" in err()
                # 4. the size: the two wavefront-level classes only, before batch == 0 and the pointers
                for n, m in ((33, 0), (40, 16), (64, 64), (128, 0), (16, 65), (1, 128)):
                    for batch, args in ((4, ptrs), (0, null), (4, null)):
                        for T in (1, MAX_RHS):
                            assert call(Desc(n, m, batch, 0, 0, 0.0), T, shared, args) == UNSUPPORTED, (name, n, m)
                            assert b"n<=32" in err() and b"m<=64" in err()
                # 5. batch 0 is a no-op before the pointers are looked at
                for n, m in ((1, 0), (16, 32), (17, 0), (32, 64)):
                    for T in (1, MAX_RHS):
                        assert call(Desc(n, m, 0, 0, 0, 0.0), T, shared, null) == 0, (name, n, m)
                # 6. missing pointers, at both kernel classes: bfac and gx, active when m > 0 ...
                for n, m in ((16, 32), (5, 3), (20, 40), (32, 64), (3, 0), (17, 0)):
                    for k in (F_, FGX_) + ((FACT_,) if m else ()):
                        args = list(ptrs)
                        args[k] = None
                        assert call(Desc(n, m, 4, 0, 0, 0.0), 2, shared, args) == INVALID, (name, n, m, k)
                        assert b"required" in err()
                    # ... and at least one output (at m == 0, gb is none)
                    args = list(ptrs)
                    args[FGF_] = args[FGB_] = None
                    assert call(Desc(n, m, 4, 0, 0, 0.0), 2, shared, args) == INVALID, (name, n, m)
                    assert b"at least one" in err()
                args = list(ptrs)
                args[FGF_] = None
                assert call(Desc(3, 0, 4, 0, 0, 0.0), 2, shared, args) == INVALID and b"at least one" in err(), name
            # 3'. a bit of `shared` other than QPB_SHARED_RHS: after the flags', before the size's and batch == 0
            for shared in (SHARED_H, SHARED_A, 3, 5, 8, -1):
                assert call(Desc(16, 32, 4, 0, 0, 0.0), 1, shared, ptrs) == INVALID, (name, shared)
                assert b"shared" in err()
                assert call(Desc(33, 64, 4, 0, 0, 0.0), 1, shared, ptrs) == INVALID and b"shared" in err()
                assert call(Desc(16, 32, 0, 0, 0, 0.0), 1, shared, null) == INVALID and b"shared" in err()
                assert call(Desc(16, 32, 4, 0, FLAG_MIXED, 0.0), 1, shared, ptrs) == INVALID and b"flags" in err()
        # 7. the alignment of the device buffer, after the pointers and before the device
        for n, m in ((16, 32), (20, 40), (3, 0)):
            args = list(ptrs)
            args[F_] = _aligned16(buf, 8)
            d = Desc(n, m, 4, 0, 0, 0.0)
            assert lib.qpb_solve_factored_backward_multi(ctypes.byref(d), *args[:3], 3, 0, *args[3:], None) == INVALID
            assert b"16-byte" in err()
            args[FGX_] = None
            assert lib.qpb_solve_factored_backward_multi(ctypes.byref(d), *args[:3], 3, 0, *args[3:], None) == INVALID
            assert b"required" in err()
    if not _device_present():
        # 8. a valid call with no device fails loudly last: status NULL, glam given or not, any one output
        ptrs = [p] * 7
        for n, m in ((16, 32), (5, 3), (20, 40), (32, 64), (3, 0)):
            d = Desc(n, m, 4, 0, 0, 0.0)
            for shared in (0, SHARED_RHS):
                for glam in (p, None):
                    for only in (FGF_, FGB_) if m else (FGF_,):
                        args = list(ptrs)
                        args[FST_], args[FGM_] = None, glam
                        args[FGF_] = p if only == FGF_ else None
                        args[FGB_] = p if only == FGB_ else None
                        for name, call in _factored_calls(lib):
                            assert call(d, MAX_RHS, shared, args) == NO_DEVICE, (name, n, m)
                            assert b"no HIP device" in err()
        # max_iter and feas_tol are ignored
        assert _factored_calls(lib)[0][1](Desc(16, 32, 4, -3, 0, -1.0), 1, 0, ptrs) == NO_DEVICE


def test_box_argument_errors_without_gpu():
    lib = _lib()
    err = lib.qpb_last_error
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 1)  # misaligned: nothing is read before the checks are through
    null = [None] * 8
    for glam in (p, None, odd):
        ptrs = [p] * 8
        ptrs[GM_] = glam
        for name, call in _box_calls(lib):
            for shared in (0, SHARED_H, SHARED_RHS, SHARED_H | SHARED_RHS):
                # 1. the descriptor, as qpb_solve_box checks it: check_desc ...
                assert call(Desc(0, 0, 4, 0, 0, 0.0), shared, 1, null) == INVALID, name
                assert call(Desc(129, 258, 4, 0, 0, 0.0), shared, 1, null) == UNSUPPORTED, name
                assert b"n<=32" not in err()  # the build's limit, not this call's
                assert call(Desc(16, 32, -1, 0, 0, 0.0), shared, 1, null) == INVALID, name
                # 2. ... then m == 2n, before the flags, the shared bits, nrhs, the size and batch == 0
                for n, m, flags, batch in ((16, 31, 0, 4), (16, 0, 0, 4), (16, 33, FLAG_MIXED, 4), (48, 95, 0, 4),
                                           (5, 9, 0, 0), (33, 64, 4, 0)):
                    for T in (1, 0):
                        assert call(Desc(n, m, batch, 0, flags, 0.0), shared, T, null) == INVALID, (name, n, m)
                        assert b"2n" in err() and b"flags" not in err() and b"nrhs" not in err()
                    assert call(Desc(n, m, batch, 0, flags, 0.0), 8, 1, null) == INVALID and b"2n" in err()
                # 3. the flags: none selects anything here, also above the size limit
                for flags in (FLAG_DIAG_L2, FLAG_MIXED, FLAG_DIAG_WAVE, 4):
                    for n in (16, 20, 48):
                        for batch, args in ((4, ptrs), (0, null)):
                            assert call(Desc(n, 2 * n, batch, 0, flags, 0.0), shared, 1, args) == INVALID, (name, flags)
                            assert b"flags" in err() and b"backward_multi" in err()
                # ... nrhs, likewise, after the flags
                for T in (0, -1, MAX_RHS + 1):
                    for n, batch, args in ((16, 4, ptrs), (48, 4, ptrs), (16, 0, null)):
                        assert call(Desc(n, 2 * n, batch, 0, 0, 0.0), shared, T, args) == INVALID, (name, T)
                        assert b"nrhs" in err() and b"256" in err()
                    assert call(Desc(16, 32, 4, 0, FLAG_MIXED, 0.0), shared, T, ptrs) == INVALID and b"flags" in err()
                # 4. the size: the two wavefront-level classes only, before batch == 0 and the pointers
                for n in (33, 40, 64, 128):
                    for batch, args in ((4, ptrs), (0, null), (4, null)):
                        for T in (1, MAX_RHS):
                            assert call(Desc(n, 2 * n, batch, 0, 0, 0.0), shared, T, args) == UNSUPPORTED, (name, n)
                            assert b"n<=32" in err()
                # 5. batch 0 is a no-op before the pointers are looked at
                for n in (1, 16, 17, 32):
                    for T in (1, MAX_RHS):
                        assert call(Desc(n, 2 * n, 0, 0, 0, 0.0), shared, T, null) == 0, (name, n)
                # 6. missing pointers, at both kernel classes: H, active and gx ...
                for n in (1, 16, 20, 32):
                    for k in (H_, ACT_, GX_):
                        args = list(ptrs)
                        args[k] = None
                        assert call(Desc(n, 2 * n, 4, 0, 0, 0.0), shared, 2, args) == INVALID, (name, n, k)
                        assert b"required" in err()
                    # ... and at least one output
                    args = list(ptrs)
                    for k in BOX_OUTPUTS:
                        args[k] = None
                    assert call(Desc(n, 2 * n, 4, 0, 0, 0.0), shared, 2, args) == INVALID, (name, n)
                    assert b"at least one" in err()
            # 3'. a bit of `shared` outside QPB_SHARED_H | QPB_SHARED_RHS: after the flags', before the size's
            for shared in (SHARED_A, 3, 6, 8, -1):
                assert call(Desc(16, 32, 4, 0, 0, 0.0), shared, 1, ptrs) == INVALID, (name, shared)
                assert b"shared" in err()
                assert call(Desc(33, 66, 4, 0, 0, 0.0), shared, 1, ptrs) == INVALID and b"shared" in err()
                assert call(Desc(16, 32, 0, 0, 0, 0.0), shared, 1, null) == INVALID and b"shared" in err()
                assert call(Desc(16, 32, 4, 0, FLAG_MIXED, 0.0), shared, 1, ptrs) == INVALID and b"flags" in err()
    if not _device_present():
        # 8. a valid call with no device fails loudly last: status NULL, glam given or not, any one output
        ptrs = [p] * 8
        for n in (1, 16, 20, 32):
            d = Desc(n, 2 * n, 4, 0, 0, 0.0)
            for shared in (0, SHARED_H, SHARED_RHS, SHARED_H | SHARED_RHS):
                for glam in (p, None):
                    for only in BOX_OUTPUTS:
                        args = list(ptrs)
                        args[ST_], args[GM_] = None, glam
                        for k in BOX_OUTPUTS:
                            args[k] = p if k == only else None
                        for name, call in _box_calls(lib):
                            assert call(d, shared, MAX_RHS, args) == NO_DEVICE, (name, n)
                            assert b"no HIP device" in err()
        # max_iter and feas_tol are ignored
        assert _box_calls(lib)[0][1](Desc(16, 32, 4, -3, 0, -1.0), 0, 1, ptrs) == NO_DEVICE


def test_python_binding_has_the_calls_and_checks_its_arguments():
    if os.environ.get("QPB_SANITIZED"):
        return  # imports torch
    import numpy as np
    import qpb
    torch = __import__("torch")
    for f in (qpb.solve_factored_backward_multi, qpb.solve_factored_backward_multi_host, qpb.solve_factored_tangents,
              qpb.solve_box_backward_multi, qpb.solve_box_backward_multi_host, qpb.solve_box_tangents):
        assert callable(f)
    assert (qpb.SHARED_RHS, qpb.MAX_RHS) == (SHARED_RHS, MAX_RHS)
    B, T, n, m = 3, 2, 4, 5
    z = lambda *s: torch.zeros(s, dtype=torch.float64)  # noqa: E731
    sol = qpb.Solution(None, None, torch.zeros((B, 1), dtype=torch.int32), None, None)
    # the device wrappers refuse host tensors before any call into the library
    F = qpb.BackwardFactor(z(qpb.factor_backward_doubles(n, m)), n, m, None)
    with pytest.raises(ValueError, match="CUDA"):
        qpb.solve_factored_backward_multi(F, sol, z(B, T, n), z(B, T, m))
    with pytest.raises(ValueError, match="CUDA"):
        qpb.solve_factored_tangents(F, sol, z(T, n))
    with pytest.raises(ValueError, match="CUDA"):
        qpb.solve_box_backward_multi(z(B, n, n), sol, z(B, T, n), z(B, T, 2 * n))
    with pytest.raises(ValueError, match="CUDA"):
        qpb.solve_box_tangents(z(n, n), sol, z(T, n), z(T, n), z(T, n))
    # the host wrappers check shapes, T and `need` before the library is called
    hs = qpb.Solution(None, None, np.zeros((B, 1), np.uint32), None, None)
    hF = qpb.BackwardFactor(np.zeros(qpb.factor_backward_doubles(n, m)), n, m, None)
    for gx, gl in ((np.zeros((B, T, n + 1)), None), (np.zeros((B + 1, T, n)), None), (np.zeros((B, T, n)), np.zeros((B, T, m + 1))),
                   (np.zeros((T, n)), np.zeros((B, T, m))), (np.zeros((B, T, n)), np.zeros((T, m))), (np.zeros(n), None)):
        with pytest.raises(ValueError, match="shape mismatch"):
            qpb.solve_factored_backward_multi_host(hF, hs, gx, gl)
    for T_bad in (0, MAX_RHS + 1):
        with pytest.raises(ValueError, match="right-hand sides"):
            qpb.solve_factored_backward_multi_host(hF, hs, np.zeros((B, T_bad, n)))
        with pytest.raises(ValueError, match="right-hand sides"):
            qpb.solve_box_backward_multi_host(np.zeros((n, n)), hs, np.zeros((T_bad, n)))
    with pytest.raises(ValueError, match="need"):
        qpb.solve_factored_backward_multi_host(hF, hs, np.zeros((B, T, n)), need=("H",))
    for H in (np.zeros((B, n, n)), np.zeros((n, n))):
        for gx, gl in ((np.zeros((B, T, n)), np.zeros((B, T, 2 * n + 1))), (np.zeros((B, T, n + 1)), None),
                       (np.zeros((T, n)), np.zeros((B, T, 2 * n)))):
            with pytest.raises(ValueError, match="shape mismatch"):
                qpb.solve_box_backward_multi_host(H, hs, gx, gl)
        with pytest.raises(ValueError, match="need"):
            qpb.solve_box_backward_multi_host(H, hs, np.zeros((B, T, n)), need=("H",))
    with pytest.raises(ValueError, match="shape mismatch"):
        qpb.solve_box_backward_multi_host(np.zeros((B + 1, n, n)), hs, np.zeros((B, T, n)))
    # errors of the library come back as QPBError with the code
    with pytest.raises(qpb.QPBError) as e:
        qpb.solve_box_backward_multi_host(np.zeros((B, 33, 33)), qpb.Solution(None, None, np.zeros((B, 3), np.uint32), None, None),
                                          np.zeros((B, T, 33)))
    assert e.value.code == qpb.ERR_UNSUPPORTED
