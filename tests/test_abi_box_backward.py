"""CPU tests of qpb_solve_box_backward's boundary (in the style of
test_abi_backward.py): the two entry points are exported, the launcher stays
hidden, and every argument error is returned before any device work, each with
its code, in qpb.h's order."""
import ctypes
import os
import subprocess

from conftest import ROOT

LIB = os.environ.get("QPB_LIB", os.path.join(ROOT, "embedded-qp-solver_amd", "lib", "libqpb.so"))
INVALID, UNSUPPORTED, NO_DEVICE = -1, -2, -4
FLAG_DIAG_L2, FLAG_MIXED, FLAG_DIAG_WAVE = 1, 32, 256
# H, x, active, status, gx, gH, gf, glb, gub
H_, X_, ACT_, ST_, GX_, GH_, GF_, GL_, GU_ = range(9)
OUTPUTS = (GH_, GF_, GL_, GU_)


class Desc(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("m", ctypes.c_int32), ("batch", ctypes.c_int64),
                ("max_iter", ctypes.c_int32), ("flags", ctypes.c_int32), ("feas_tol", ctypes.c_double)]


def _lib():
    lib = ctypes.CDLL(LIB)
    vp = ctypes.c_void_p
    lib.qpb_last_error.restype = ctypes.c_char_p
    lib.qpb_solve_box_backward.argtypes = [ctypes.POINTER(Desc)] + [vp] * 10
    lib.qpb_solve_box_backward_host.argtypes = [ctypes.POINTER(Desc)] + [vp] * 9
    return lib


def _device_present():
    if os.environ.get("QPB_SANITIZED"):
        return False
    import torch
    return torch.cuda.is_available()


def test_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {"qpb_solve_box_backward", "qpb_solve_box_backward_host"} <= syms
    assert not {s for s in syms if s.startswith("qpb_launch_")}


def _calls(lib):
    """Both entry points with the same (desc, nine array pointers)."""
    return (("qpb_solve_box_backward", lambda d, a: lib.qpb_solve_box_backward(ctypes.byref(d), *a, None)),
            ("qpb_solve_box_backward_host", lambda d, a: lib.qpb_solve_box_backward_host(ctypes.byref(d), *a)))


def test_argument_errors_without_gpu():
    lib = _lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    null, ptrs = [None] * 9, [p] * 9
    for name, call in _calls(lib):
        # 1. the descriptor, as qpb_solve_box checks it: check_desc ...
        assert call(Desc(0, 0, 4, 0, 0, 0.0), null) == INVALID, name
        assert call(Desc(129, 258, 4, 0, 0, 0.0), null) == UNSUPPORTED, name
        assert b"n<=32" not in lib.qpb_last_error()  # the build's limit, not this call's
        assert call(Desc(16, 32, -1, 0, 0, 0.0), null) == INVALID, name
        # ... then m == 2n, before the flags, the size and batch == 0
        for n, m, flags, batch in ((16, 31, 0, 4), (16, 0, 0, 4), (16, 33, FLAG_MIXED, 4), (48, 95, 0, 4),
                                   (5, 9, 0, 0), (33, 64, 4, 0)):
            assert call(Desc(n, m, batch, 0, flags, 0.0), null) == INVALID, (name, n, m)
            assert b"2n" in lib.qpb_last_error() and b"flags" not in lib.qpb_last_error()
        # 2. the flags: none selects anything here, also above the size limit
        for flags in (FLAG_DIAG_L2, FLAG_MIXED, FLAG_DIAG_WAVE, 4):
            for n in (16, 20, 48):
                for batch, args in ((4, ptrs), (0, null)):
                    assert call(Desc(n, 2 * n, batch, 0, flags, 0.0), args) == INVALID, (name, flags, n)
                    assert b"flags" in lib.qpb_last_error()
        # 3. the size: the two wavefront-level classes only, before batch == 0 and the pointers
        for n in (33, 40, 64, 128):
            for batch, args in ((4, ptrs), (0, null), (4, null)):
                assert call(Desc(n, 2 * n, batch, 0, 0, 0.0), args) == UNSUPPORTED, (name, n, batch)
                assert b"n<=32" in lib.qpb_last_error()
        # 4. batch 0 is a no-op before the pointers are looked at
        for n in (1, 16, 17, 32):
            assert call(Desc(n, 2 * n, 0, 0, 0, 0.0), null) == 0, (name, n)
        # 5. missing pointers, at both kernel classes: H, x, active and gx ...
        for n in (1, 16, 20, 32):
            for k in (H_, X_, ACT_, GX_):
                args = list(ptrs)
                args[k] = None
                assert call(Desc(n, 2 * n, 4, 0, 0, 0.0), args) == INVALID, (name, n, k)
                assert b"required" in lib.qpb_last_error()
            # ... and at least one output
            args = list(ptrs)
            for k in OUTPUTS:
                args[k] = None
            assert call(Desc(n, 2 * n, 4, 0, 0, 0.0), args) == INVALID, (name, n)
            assert b"at least one" in lib.qpb_last_error()
    if not _device_present():
        # 6. a valid call with no device fails loudly last: status NULL, any one output
        for n in (1, 16, 20, 32):
            d = Desc(n, 2 * n, 4, 0, 0, 0.0)
            for only in OUTPUTS:
                args = list(ptrs)
                args[ST_] = None
                for k in OUTPUTS:
                    args[k] = p if k == only else None
                assert lib.qpb_solve_box_backward(ctypes.byref(d), *args, None) == NO_DEVICE, (n, only)
                assert b"no HIP device" in lib.qpb_last_error()
                assert lib.qpb_solve_box_backward_host(ctypes.byref(d), *args) == NO_DEVICE, (n, only)
        # max_iter and feas_tol are ignored
        assert lib.qpb_solve_box_backward(ctypes.byref(Desc(16, 32, 4, -3, 0, -1.0)), *ptrs, None) == NO_DEVICE


def test_version_names_the_box_backward_kernels():
    lib = _lib()
    lib.qpb_version.restype = ctypes.c_char_p
    v = lib.qpb_version().decode()
    assert v.startswith("qpb 0.14 ") and "kkt_bwd v1.1" in v and "kkt_bwd_box v1.0" in v
    assert "gi_eq v1.0" in v and "gi_dense v11.6" in v and "gi_box v2.2" in v
    # the `;`-separated form the benchmark splits on: the token is a part's head
    inner = v.split("(", 1)[1].rsplit(")", 1)[0]
    heads = {part.split(":", 1)[0].strip() for part in inner.split(";") if ":" in part}
    assert {"kkt_bwd_box v1.0", "kkt_bwd v1.1", "gi_box v2.2", "gi_dense v11.7"} <= heads


def test_python_binding_has_the_calls():
    if os.environ.get("QPB_SANITIZED"):
        return  # imports torch
    import qpb
    assert callable(qpb.solve_box_backward) and callable(qpb.solve_box_backward_host)
    import qpb.diff
    assert callable(qpb.diff.solve_box)
    assert issubclass(qpb.diff.BoxQPFunction, __import__("torch").autograd.Function)
