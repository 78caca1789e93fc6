"""CPU tests of qpb_solve_box_backward_dual's boundary (in the style of
test_abi_box_backward.py and test_abi_backward_dual.py): the two entry points
are exported, the launchers stay hidden, and every argument error is returned
before any device work, each with its code, in qpb.h's order -- with glam given,
NULL and odd (never read: it is never required)."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT

LIB = os.environ.get("QPB_LIB", os.path.join(ROOT, "embedded-qp-solver_amd", "lib", "libqpb.so"))
INVALID, UNSUPPORTED, NO_DEVICE = -1, -2, -4
FLAG_DIAG_L2, FLAG_MIXED, FLAG_DIAG_WAVE = 1, 32, 256
SHARED_H = 1
# H, x, active, status, gx, glam, gH, gf, glb, gub
H_, X_, ACT_, ST_, GX_, GM_, GH_, GF_, GL_, GU_ = range(10)
OUTPUTS = (GH_, GF_, GL_, GU_)


class Desc(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("m", ctypes.c_int32), ("batch", ctypes.c_int64),
                ("max_iter", ctypes.c_int32), ("flags", ctypes.c_int32), ("feas_tol", ctypes.c_double)]


def _lib():
    lib = ctypes.CDLL(LIB)
    vp = ctypes.c_void_p
    lib.qpb_last_error.restype = ctypes.c_char_p
    lib.qpb_solve_box_backward_dual.argtypes = [ctypes.POINTER(Desc), ctypes.c_int32] + [vp] * 11
    lib.qpb_solve_box_backward_dual_host.argtypes = [ctypes.POINTER(Desc), ctypes.c_int32] + [vp] * 10
    return lib


def _device_present():
    if os.environ.get("QPB_SANITIZED"):
        return False
    import torch
    return torch.cuda.is_available()


def test_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {"qpb_solve_box_backward_dual", "qpb_solve_box_backward_dual_host"} <= syms
    assert not {s for s in syms if s.startswith("qpb_launch_")}


def _calls(lib):
    """Both entry points with the same (desc, shared, ten array pointers)."""
    return (("qpb_solve_box_backward_dual",
             lambda d, sh, a: lib.qpb_solve_box_backward_dual(ctypes.byref(d), sh, *a, None)),
            ("qpb_solve_box_backward_dual_host",
             lambda d, sh, a: lib.qpb_solve_box_backward_dual_host(ctypes.byref(d), sh, *a)))


def test_argument_errors_without_gpu():
    lib = _lib()
    err = lib.qpb_last_error
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 1)  # misaligned: nothing is read before the checks are through
    null = [None] * 10
    for glam in (p, None, odd):
        ptrs = [p] * 10
        ptrs[GM_] = glam
        for name, call in _calls(lib):
            for shared in (0, SHARED_H):
                # 1. the descriptor, as qpb_solve_box checks it: check_desc ...
                assert call(Desc(0, 0, 4, 0, 0, 0.0), shared, null) == INVALID, name
                assert call(Desc(129, 258, 4, 0, 0, 0.0), shared, null) == UNSUPPORTED, name
                assert b"n<=32" not in err()  # the build's limit, not this call's
                assert call(Desc(16, 32, -1, 0, 0, 0.0), shared, null) == INVALID, name
                # ... then m == 2n, before the flags, the shared bits, the size and batch == 0
                for n, m, flags, batch in ((16, 31, 0, 4), (16, 0, 0, 4), (16, 33, FLAG_MIXED, 4), (48, 95, 0, 4),
                                           (5, 9, 0, 0), (33, 64, 4, 0)):
                    assert call(Desc(n, m, batch, 0, flags, 0.0), shared, null) == INVALID, (name, n, m)
                    assert b"2n" in err() and b"flags" not in err()
                    assert call(Desc(n, m, batch, 0, flags, 0.0), 4, null) == INVALID and b"2n" in err()
                # 2. the flags: none selects anything here, also above the size limit
                for flags in (FLAG_DIAG_L2, FLAG_MIXED, FLAG_DIAG_WAVE, 4):
                    for n in (16, 20, 48):
                        for batch, args in ((4, ptrs), (0, null)):
                            assert call(Desc(n, 2 * n, batch, 0, flags, 0.0), shared, args) == INVALID, (name, flags, n)
                            assert b"flags" in err()
                # 3. the size: the two wavefront-level classes only, before batch == 0 and the pointers
                for n in (33, 40, 64, 128):
                    for batch, args in ((4, ptrs), (0, null), (4, null)):
                        assert call(Desc(n, 2 * n, batch, 0, 0, 0.0), shared, args) == UNSUPPORTED, (name, n, batch)
                        assert b"n<=32" in err()
                # 4. batch 0 is a no-op before the pointers are looked at
                for n in (1, 16, 17, 32):
                    assert call(Desc(n, 2 * n, 0, 0, 0, 0.0), shared, null) == 0, (name, n)
                # 5. missing pointers, at both kernel classes: H, x, active and gx ...
                for n in (1, 16, 20, 32):
                    for k in (H_, X_, ACT_, GX_):
                        args = list(ptrs)
                        args[k] = None
                        assert call(Desc(n, 2 * n, 4, 0, 0, 0.0), shared, args) == INVALID, (name, n, k)
                        assert b"required" in err()
                    # ... and at least one output
                    args = list(ptrs)
                    for k in OUTPUTS:
                        args[k] = None
                    assert call(Desc(n, 2 * n, 4, 0, 0, 0.0), shared, args) == INVALID, (name, n)
                    assert b"at least one" in err()
            # 2'. a bit of `shared` other than QPB_SHARED_H: after the flags', before the size's and batch == 0
            for shared in (2, 3, 4, -1):
                assert call(Desc(16, 32, 4, 0, 0, 0.0), shared, ptrs) == INVALID, (name, shared)
                assert b"shared" in err()
                assert call(Desc(33, 66, 4, 0, 0, 0.0), shared, ptrs) == INVALID and b"shared" in err()
                assert call(Desc(16, 32, 0, 0, 0, 0.0), shared, null) == INVALID and b"shared" in err()
                assert call(Desc(16, 32, 4, 0, FLAG_MIXED, 0.0), shared, ptrs) == INVALID and b"flags" in err()
    if not _device_present():
        # 6. a valid call with no device fails loudly last: status NULL, glam given or not, any one output
        ptrs = [p] * 10
        for n in (1, 16, 20, 32):
            d = Desc(n, 2 * n, 4, 0, 0, 0.0)
            for shared in (0, SHARED_H):
                for glam in (p, None):
                    for only in OUTPUTS:
                        args = list(ptrs)
                        args[ST_], args[GM_] = None, glam
                        for k in OUTPUTS:
                            args[k] = p if k == only else None
                        assert lib.qpb_solve_box_backward_dual(ctypes.byref(d), shared, *args, None) == NO_DEVICE
                        assert b"no HIP device" in err()
                        assert lib.qpb_solve_box_backward_dual_host(ctypes.byref(d), shared, *args) == NO_DEVICE
        # max_iter and feas_tol are ignored
        assert lib.qpb_solve_box_backward_dual(ctypes.byref(Desc(16, 32, 4, -3, 0, -1.0)), 0, *ptrs, None) == NO_DEVICE


def test_python_binding_has_the_calls_and_checks_its_arguments():
    if os.environ.get("QPB_SANITIZED"):
        return  # imports torch
    import numpy as np
    import qpb
    import qpb.diff
    torch = __import__("torch")
    for f in (qpb.solve_box_backward_dual, qpb.solve_box_backward_dual_host, qpb.solve_box_tangent):
        assert callable(f)
    assert issubclass(qpb.diff.BoxDualQPFunction, torch.autograd.Function)
    B, n = 3, 4
    z = lambda *s: torch.zeros(s, dtype=torch.float64)  # noqa: E731
    sol = qpb.Solution(z(B, n), None, torch.zeros((B, 1), dtype=torch.int32), None, None)
    # the device wrappers refuse host tensors before any call into the library
    with pytest.raises(ValueError, match="CUDA"):
        qpb.solve_box_backward_dual(z(B, n, n), sol, z(B, n), z(B, 2 * n))
    with pytest.raises(ValueError, match="CUDA"):
        qpb.solve_box_tangent(z(n, n), sol, z(B, n), z(B, n), z(B, n))
    with pytest.raises(ValueError, match="prefactor"):
        qpb.diff.solve_box_dual(z(B, n, n), z(B, n), prefactor=True)
    # the host wrapper checks shapes and `need` before the library is called
    hs = qpb.Solution(np.zeros((B, n)), None, np.zeros((B, 1), np.uint32), None, None)
    for H in (np.zeros((B, n, n)), np.zeros((n, n))):
        with pytest.raises(ValueError, match="shape mismatch"):
            qpb.solve_box_backward_dual_host(H, hs, np.zeros((B, n)), np.zeros((B, 2 * n + 1)))
        with pytest.raises(ValueError, match="need"):
            qpb.solve_box_backward_dual_host(H, hs, np.zeros((B, n)), np.zeros((B, 2 * n)), need=("x",))
    # errors of the library come back as QPBError with the code
    with pytest.raises(qpb.QPBError) as e:
        qpb.solve_box_backward_dual_host(np.zeros((B, 33, 33)), qpb.Solution(np.zeros((B, 33)), None, np.zeros((B, 3), np.uint32), None, None),
                                         np.zeros((B, 33)), np.zeros((B, 66)))
    assert e.value.code == qpb.ERR_UNSUPPORTED
