"""CPU tests of the boundary of qpb_solve_range_box_backward (in the style of
test_abi_range_box.py): the two entry points are exported, the launchers stay
hidden, and every argument error is returned before any device work, each with
its code, in qpb.h's order.  desc->m is mg, the number of general rows."""
import ctypes
import os
import subprocess

from conftest import ROOT

LIB = os.environ.get("QPB_LIB", os.path.join(ROOT, "embedded-qp-solver_amd", "lib", "libqpb.so"))
INVALID, UNSUPPORTED, NO_DEVICE = -1, -2, -4
FLAG_DIAG_L2, FLAG_MIXED, FLAG_DIAG_WAVE = 1, 32, 256
# H, G, x, lam, active, lower, status, gx, glam, gH, gf, gG, gbl, gbu, glb, gub
H_, G_, X_, LAM_, ACT_, LOW_, ST_, GX_, GLAM_, GH_, GF_, GG_, GBL_, GBU_, GLB_, GUB_ = range(16)
OUTS = (GH_, GF_, GG_, GBL_, GBU_, GLB_, GUB_)


class Desc(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("m", ctypes.c_int32), ("batch", ctypes.c_int64),
                ("max_iter", ctypes.c_int32), ("flags", ctypes.c_int32), ("feas_tol", ctypes.c_double)]


def _lib():
    lib = ctypes.CDLL(LIB)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.qpb_last_error.restype = ctypes.c_char_p
    lib.qpb_solve_range_box_backward.argtypes = [ctypes.POINTER(Desc), i32] + [vp] * 17
    lib.qpb_solve_range_box_backward_host.argtypes = [ctypes.POINTER(Desc), i32] + [vp] * 16
    return lib


def _device_present():
    if os.environ.get("QPB_SANITIZED"):
        return False
    import torch
    return torch.cuda.is_available()


def test_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {"qpb_solve_range_box_backward", "qpb_solve_range_box_backward_host"} <= syms
    assert not {s for s in syms if s.startswith("qpb_launch_")}


def _calls(lib):
    return (("qpb_solve_range_box_backward",
             lambda d, sh, a: lib.qpb_solve_range_box_backward(ctypes.byref(d), sh, *a, None)),
            ("qpb_solve_range_box_backward_host",
             lambda d, sh, a: lib.qpb_solve_range_box_backward_host(ctypes.byref(d), sh, *a)))


def _without(ptrs, *drop):
    args = list(ptrs)
    for k in drop:
        args[k] = None
    return args


def test_argument_errors_without_gpu():
    lib = _lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 1)  # a misaligned pointer: never dereferenced before the device check
    null, ptrs = [None] * 16, [p] * 16
    err = lib.qpb_last_error
    for name, call in _calls(lib):
        for sh in (0, 1, 2, 3):
            # 1. the descriptor's own rules come first, as in qpb_solve, with m = mg
            assert call(Desc(0, 0, 4, 0, 0, 0.0), sh, null) == INVALID, name
            assert call(Desc(16, -1, 4, 0, 0, 0.0), sh, null) == INVALID, name
            assert call(Desc(129, 32, 4, 0, 0, 0.0), sh, null) == UNSUPPORTED, name
            assert b"range_box" not in err()  # the descriptor's message, not this call's
            assert call(Desc(16, 16, -1, 0, 0, 0.0), sh, null) == INVALID, name
            # 2. then the flags, also above the size limit and with a bad `shared`
            for flags in (FLAG_DIAG_L2, FLAG_MIXED, FLAG_DIAG_WAVE, 4):
                for n, mg in ((16, 16), (48, 96)):
                    assert call(Desc(n, mg, 4, 0, flags, 0.0), sh | 4, ptrs) == INVALID, (name, flags, n, mg)
                    assert b"flags" in err() and b"range_box_backward" in err()
        # ... the bits of `shared`, before the size and batch == 0
        for sh in (4, 7, 8, -1, 1 << 30):
            for n, mg, batch in ((16, 16, 4), (48, 96, 4), (16, 16, 0)):
                assert call(Desc(n, mg, batch, 0, 0, 0.0), sh, null) == INVALID, (name, sh, n, mg)
                assert b"QPB_SHARED_H" in err()
        # 3. then the size, whatever is shared: n <= 32 and mg + n <= 64, a message that names the
        # call and the limit, before batch == 0 and the pointers
        for sh in (0, 1, 2, 3):
            for n, mg in ((33, 0), (32, 33), (16, 49), (33, 1), (1, 64), (20, 45), (128, 128), (64, 0)):
                for batch, args in ((4, ptrs), (0, null), (4, null)):
                    assert call(Desc(n, mg, batch, 0, 0, 0.0), sh, args) == UNSUPPORTED, (name, n, mg, sh)
                    assert b"range_box_backward" in err() and b"n<=32" in err() and b"mg+n<=64" in err()
            # (129, 32) is the descriptor's own limit, with its message
            assert call(Desc(129, 32, 4, 0, 0, 0.0), sh, ptrs) == UNSUPPORTED and b"range_box" not in err(), name
        # 4. batch 0 is a no-op before the pointers are looked at
        for sh in (0, 1, 2, 3):
            for n, mg in ((16, 16), (20, 40), (32, 32), (3, 0), (1, 63)):
                assert call(Desc(n, mg, 0, 0, 0, 0.0), sh, null) == 0, (name, n, mg, sh)
        # 5. missing pointers: H, x, lam, active and gx always (status and glam may be NULL) ...
        for sh in (0, 1, 2, 3):
            for n, mg in ((16, 16), (20, 33), (3, 0)):
                for k in (H_, X_, LAM_, ACT_, GX_):
                    for base in (ptrs, [odd] * 16):
                        assert call(Desc(n, mg, 4, 0, 0, 0.0), sh, _without(base, k)) == INVALID, (name, n, mg, k)
                        assert b"are required" in err()
            # ... G when mg > 0
            for n, mg in ((16, 16), (20, 33), (1, 1)):
                assert call(Desc(n, mg, 4, 0, 0, 0.0), sh, _without(ptrs, G_)) == INVALID, (name, n, mg)
                assert b"G is required" in err()
            # ... lower when gbl or glb is given
            for n, mg in ((16, 16), (20, 33), (3, 0)):
                for keep in ((GBL_,), (GLB_,), (GBL_, GLB_)):
                    drop = [LOW_] + [k for k in (GBL_, GLB_) if k not in keep]
                    assert call(Desc(n, mg, 4, 0, 0, 0.0), sh, _without(ptrs, *drop)) == INVALID, (name, n, mg, keep)
                    assert b"lower is required" in err()
            # ... and at least one output; at mg == 0 gG, gbl and gbu do not count
            for n, mg in ((16, 16), (20, 33), (3, 0)):
                assert call(Desc(n, mg, 4, 0, 0, 0.0), sh, _without(ptrs, *OUTS)) == INVALID, (name, n, mg)
                assert b"at least one of gH, gf, gG, gbl, gbu, glb and gub" in err()
            assert call(Desc(3, 0, 4, 0, 0, 0.0), sh, _without(ptrs, GH_, GF_, GLB_, GUB_)) == INVALID, name
            assert b"at least one of" in err()
    if not _device_present():
        # 6. a valid call with no device fails loudly last: every output alone, status and glam NULL
        for sh in (0, 1, 2, 3):
            for n, mg in ((16, 16), (20, 40), (32, 32), (1, 1), (12, 20)):
                for keep in OUTS:
                    args = _without(ptrs, ST_, GLAM_, *(k for k in OUTS if k != keep))
                    d = Desc(n, mg, 4, 0, 0, 0.0)
                    assert lib.qpb_solve_range_box_backward(ctypes.byref(d), sh, *args, None) == NO_DEVICE, (n, mg, sh, keep)
                    assert b"no HIP device" in err()
                    assert lib.qpb_solve_range_box_backward_host(ctypes.byref(d), sh, *args) == NO_DEVICE, (n, mg, sh, keep)
                # lower NULL without gbl and glb: everything routed goes to the upper arrays
                args = _without(ptrs, LOW_, GBL_, GLB_)
                d = Desc(n, mg, 4, 0, 0, 0.0)
                assert lib.qpb_solve_range_box_backward(ctypes.byref(d), sh, *args, None) == NO_DEVICE, (n, mg, sh)
                assert lib.qpb_solve_range_box_backward_host(ctypes.byref(d), sh, *args) == NO_DEVICE, (n, mg, sh)
        # mg == 0: G may be NULL, and the rows' outputs with it
        args = _without(ptrs, G_, GG_, GBL_, GBU_)
        for n in (1, 16, 17, 32):
            d = Desc(n, 0, 4, 0, 0, 0.0)
            assert lib.qpb_solve_range_box_backward(ctypes.byref(d), 3, *args, None) == NO_DEVICE
            assert lib.qpb_solve_range_box_backward_host(ctypes.byref(d), 0, *args) == NO_DEVICE


def test_version_names_the_form_beside_the_old_ones():
    lib = _lib()
    lib.qpb_version.restype = ctypes.c_char_p
    v = lib.qpb_version().decode()
    assert v.startswith("qpb 0.14 ")
    tokens = [t.strip() for t in v[v.index("(") + 1:].split(";")]
    assert any(t.startswith("kkt_bwd_range_box v1.0:") for t in tokens)
    for old in ("gfx950", "gi_dense v11.7", "gi_box v2.2", "gi_wave v6.7", "gi_gram v4.5", "ref v6", "gi_eq v1.0",
                "kkt_bwd v1.1", "kkt_bwd_box v1.0", "gi_shared v1.0", "kkt_bwd_sum v1.0", "gi_range v1.0:",
                "gi_fact v1.0", "gi_rfact v1.0", "box_shared v1.0", "box_fact v1.0", "gi_range_box v1.0:"):
        assert any(t.startswith(old) for t in tokens), old


def test_python_binding_has_the_calls():
    if os.environ.get("QPB_SANITIZED"):
        return  # imports torch
    import qpb
    for name in ("solve_range_box_backward", "solve_range_box_backward_host", "solve_range_box"):
        assert callable(getattr(qpb, name)), name
    assert qpb.RANGE_BOX_NEED_ALL == ("H", "f", "G", "bl", "bu", "lb", "ub")
    assert len(qpb._lib.qpb_solve_range_box_backward.argtypes) == 19
    assert len(qpb._lib.qpb_solve_range_box_backward_host.argtypes) == 18
    import inspect
    import qpb.diff
    assert callable(qpb.diff.solve_range_box_dual) and callable(qpb.diff.solve_range_box)
    # the autograd function no longer assembles [G; I]
    src = inspect.getsource(qpb.diff.RangeBoxQPFunction) + inspect.getsource(qpb.diff._range_box_backward)
    assert "torch.cat" not in src and "torch.eye" not in src
