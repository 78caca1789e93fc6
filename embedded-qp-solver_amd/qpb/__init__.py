"""qpb -- Python host binding of the batched MI355X QP solver (include/qpb.h).

Thin ctypes layer over ``lib/libqpb.so`` (built by ``make -C
embedded-qp-solver_amd``).  Device memory and streams are PyTorch-ROCm tensors
and streams; every solve runs in the HIP kernels of the library.  There is no
CPU fallback: importing this module fails loudly when the library is missing,
and solving fails when no HIP device is present.

The reference's single-QP C API (qp.h / qp_solvers.h) is the C
compat layer in include/compat/; this module mirrors the batched C-ABI:

    solve(H, f, A, b)          -> qpb_solve       (active set, m > 0)
    solve(H, f)                -> qpb_solve, m=0  (test/qp_ref.py:35 semantics)
    solve_eq(H, f, A, b, meq)  -> qpb_solve_eq    (rows 0 .. meq-1 of A are equalities)
    solve_backward(H, A, sol, gx) -> qpb_solve_backward (gradients of a solve; autograd: qpb.diff)
    solve_shared(H, f, A, b, meq) -> qpb_solve_shared (a 2-D H and / or A: one matrix for the whole batch)
    solve_shared_backward(H, A, sol, gx) -> qpb_solve_shared_backward (a shared operand's gradient summed over the batch)
    solve_backward_dual(H, A, sol, gx, glam) -> qpb_solve_backward_dual (a cotangent on lam as well; autograd: qpb.diff.solve_dual)
    solve_tangent(H, A, sol, df, db) -> qpb_solve_backward_dual (the tangent of (x*, lam*) along (df, db))
    solve_box_backward(H, sol, gx) -> qpb_solve_box_backward (gradients of a box solve, n <= 32)
    solve_box_shared(H, f, lb, ub) -> qpb_solve_box_shared (a box solve with ONE H (n, n) for the whole batch, n <= 128)
    solve_box_shared_backward(H, sol, gx) -> qpb_solve_box_shared_backward (its gradients, gH (n, n) summed over the batch, n <= 32)
    solve_range(H, f, A, bl, bu, meq) -> qpb_solve_range (two-sided rows bl <= A x <= bu, signed lam; n <= 32, m <= 64)
    solve_range_box(H, f, G, bl, bu, lb, ub, meq) -> qpb_solve_range_box (those rows beside lb <= x <= ub; mg + n <= 64)
    ref_solve(mode, P, q, x0)  -> qpb_ref_solve   (qp_solvers.c replicas)
    qf_eval(P, q, r, x)        -> qpb_qf_eval     (qp.c:9-27)
    ref_generate(n, B, seed)   -> qpb_ref_generate (the reference generator, bit for bit)
    generate(n, B, seed)       -> qpb_generate     (Philox benchmark families)
"""
from __future__ import annotations

import ctypes
import os
from typing import NamedTuple

HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(HERE)
LIB_PATH = os.environ.get("QPB_LIB", os.path.join(PKG_ROOT, "lib", "libqpb.so"))

if not os.path.exists(LIB_PATH):
    raise ImportError(f"qpb: {LIB_PATH} not found -- build it with `make -C {PKG_ROOT}` "
                      "(there is no CPU fallback)")

_lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)

# status codes (qpb_status)
OK, MAX_ITER, NOT_SPD, INFEASIBLE, NUMERICAL = 0, 1, 2, 3, 4
STATUS_NAMES = {OK: "OK", MAX_ITER: "MAX_ITER", NOT_SPD: "NOT_SPD", INFEASIBLE: "INFEASIBLE", NUMERICAL: "NUMERICAL"}
# error codes (qpb_error)
ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_HIP, ERR_NO_DEVICE = -1, -2, -3, -4
# reference modes (qpb_ref_mode)
REF_NEWTON, REF_ADMM, REF_GD = 1, 2, 3
MAX_N, MAX_M = 128, 256
REF_MAX_N = 1024  # qpb_ref_solve / qpb_matrix_invert (QPB_REF_MAX_N)
# qpb_desc.flags (include/qpb.h)
FLAG_DIAG_L2, FLAG_DIAG_MALL = 1, 16
FLAG_MIXED, FLAG_DIAG_NO_REDO = 32, 64
# the `shared` argument of qpb_solve_shared / qpb_solve_shared_backward
SHARED_H, SHARED_A = 1, 2
SHARED_RHS = 4  # the *_multi calls: gx and glam are ONE set of T right-hand sides for the whole batch
MAX_RHS = 256
FLAG_DIAG_WAVE = 256  # n <= 16 solved by the one-QP-per-wavefront kernel (lockstep endpoint; measurement only)
STATUS_REDO = 100  # internal: a QP the mixed kernel leaves to the fp64 re-solve (FLAG_DIAG_NO_REDO only)


class Desc(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("m", ctypes.c_int32), ("batch", ctypes.c_int64),
                ("max_iter", ctypes.c_int32), ("flags", ctypes.c_int32), ("feas_tol", ctypes.c_double)]


class RefDesc(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("mode", ctypes.c_int32), ("batch", ctypes.c_int64),
                ("iterations", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("box_min", ctypes.c_double), ("box_max", ctypes.c_double)]


_vp = ctypes.c_void_p
_lib.qpb_solve.argtypes = [ctypes.POINTER(Desc)] + [_vp] * 10
_lib.qpb_solve.restype = ctypes.c_int
_lib.qpb_solve_host.argtypes = [ctypes.POINTER(Desc)] + [_vp] * 9
_lib.qpb_solve_host.restype = ctypes.c_int
_lib.qpb_solve_eq.argtypes = [ctypes.POINTER(Desc), ctypes.c_int32] + [_vp] * 10
_lib.qpb_solve_eq.restype = ctypes.c_int
_lib.qpb_solve_eq_host.argtypes = [ctypes.POINTER(Desc), ctypes.c_int32] + [_vp] * 9
_lib.qpb_solve_eq_host.restype = ctypes.c_int
_lib.qpb_solve_backward.argtypes = [ctypes.POINTER(Desc)] + [_vp] * 12
_lib.qpb_solve_backward.restype = ctypes.c_int
_lib.qpb_solve_backward_host.argtypes = [ctypes.POINTER(Desc)] + [_vp] * 11
_lib.qpb_solve_backward_host.restype = ctypes.c_int
_lib.qpb_solve_shared.argtypes = [ctypes.POINTER(Desc), ctypes.c_int32, ctypes.c_int32] + [_vp] * 10
_lib.qpb_solve_shared.restype = ctypes.c_int
_lib.qpb_solve_shared_host.argtypes = [ctypes.POINTER(Desc), ctypes.c_int32, ctypes.c_int32] + [_vp] * 9
_lib.qpb_solve_shared_host.restype = ctypes.c_int
_lib.qpb_factor_doubles.argtypes = [ctypes.c_int32, ctypes.c_int32]
_lib.qpb_factor_doubles.restype = ctypes.c_int64
_lib.qpb_factor_shared.argtypes = [ctypes.c_int32, ctypes.c_int32] + [_vp] * 5
_lib.qpb_factor_shared.restype = ctypes.c_int
_lib.qpb_factor_shared_host.argtypes = [ctypes.c_int32, ctypes.c_int32] + [_vp] * 4
_lib.qpb_factor_shared_host.restype = ctypes.c_int
_lib.qpb_solve_factored.argtypes = [ctypes.POINTER(Desc), ctypes.c_int32] + [_vp] * 9
_lib.qpb_solve_factored.restype = ctypes.c_int
_lib.qpb_solve_factored_host.argtypes = [ctypes.POINTER(Desc), ctypes.c_int32] + [_vp] * 8
_lib.qpb_solve_factored_host.restype = ctypes.c_int
_lib.qpb_solve_shared_backward.argtypes = [ctypes.POINTER(Desc), ctypes.c_int32] + [_vp] * 12
_lib.qpb_solve_shared_backward.restype = ctypes.c_int
_lib.qpb_solve_shared_backward_host.argtypes = [ctypes.POINTER(Desc), ctypes.c_int32] + [_vp] * 11
_lib.qpb_solve_shared_backward_host.restype = ctypes.c_int
_lib.qpb_solve_backward_dual.argtypes = [ctypes.POINTER(Desc), ctypes.c_int32] + [_vp] * 13
_lib.qpb_solve_backward_dual.restype = ctypes.c_int
_lib.qpb_solve_backward_dual_host.argtypes = [ctypes.POINTER(Desc), ctypes.c_int32] + [_vp] * 12
_lib.qpb_solve_backward_dual_host.restype = ctypes.c_int
_lib.qpb_factor_backward_doubles.argtypes = [ctypes.c_int32, ctypes.c_int32]
_lib.qpb_factor_backward_doubles.restype = ctypes.c_int64
_lib.qpb_factor_shared_backward.argtypes = [ctypes.c_int32, ctypes.c_int32] + [_vp] * 5
_lib.qpb_factor_shared_backward.restype = ctypes.c_int
_lib.qpb_factor_shared_backward_host.argtypes = [ctypes.c_int32, ctypes.c_int32] + [_vp] * 4
_lib.qpb_factor_shared_backward_host.restype = ctypes.c_int
_lib.qpb_solve_factored_backward.argtypes = [ctypes.POINTER(Desc)] + [_vp] * 11
_lib.qpb_solve_factored_backward.restype = ctypes.c_int
_lib.qpb_solve_factored_backward_host.argtypes = [ctypes.POINTER(Desc)] + [_vp] * 10
_lib.qpb_solve_factored_backward_host.restype = ctypes.c_int
_lib.qpb_solve_factored_backward_dual.argtypes = [ctypes.POINTER(Desc)] + [_vp] * 12
_lib.qpb_solve_factored_backward_dual.restype = ctypes.c_int
_lib.qpb_solve_factored_backward_dual_host.argtypes = [ctypes.POINTER(Desc)] + [_vp] * 11
_lib.qpb_solve_factored_backward_dual_host.restype = ctypes.c_int
_lib.qpb_solve_range.argtypes = [ctypes.POINTER(Desc), ctypes.c_int32, ctypes.c_int32] + [_vp] * 12
_lib.qpb_solve_range.restype = ctypes.c_int
_lib.qpb_solve_range_host.argtypes = [ctypes.POINTER(Desc), ctypes.c_int32, ctypes.c_int32] + [_vp] * 11
_lib.qpb_solve_range_host.restype = ctypes.c_int
_lib.qpb_solve_range_box.argtypes = [ctypes.POINTER(Desc), ctypes.c_int32, ctypes.c_int32] + [_vp] * 14
_lib.qpb_solve_range_box.restype = ctypes.c_int
_lib.qpb_solve_range_box_host.argtypes = [ctypes.POINTER(Desc), ctypes.c_int32, ctypes.c_int32] + [_vp] * 13
_lib.qpb_solve_range_box_host.restype = ctypes.c_int
_lib.qpb_solve_range_box_backward.argtypes = [ctypes.POINTER(Desc), ctypes.c_int32] + [_vp] * 17
_lib.qpb_solve_range_box_backward.restype = ctypes.c_int
_lib.qpb_solve_range_box_backward_host.argtypes = [ctypes.POINTER(Desc), ctypes.c_int32] + [_vp] * 16
_lib.qpb_solve_range_box_backward_host.restype = ctypes.c_int
_lib.qpb_solve_range_factored.argtypes = [ctypes.POINTER(Desc), ctypes.c_int32] + [_vp] * 11
_lib.qpb_solve_range_factored.restype = ctypes.c_int
_lib.qpb_solve_range_factored_host.argtypes = [ctypes.POINTER(Desc), ctypes.c_int32] + [_vp] * 10
_lib.qpb_solve_range_factored_host.restype = ctypes.c_int
_lib.qpb_solve_box.argtypes = [ctypes.POINTER(Desc)] + [_vp] * 10
_lib.qpb_solve_box.restype = ctypes.c_int
_lib.qpb_solve_box_backward.argtypes = [ctypes.POINTER(Desc)] + [_vp] * 10
_lib.qpb_solve_box_backward.restype = ctypes.c_int
_lib.qpb_solve_box_backward_host.argtypes = [ctypes.POINTER(Desc)] + [_vp] * 9
_lib.qpb_solve_box_backward_host.restype = ctypes.c_int
_lib.qpb_solve_box_shared.argtypes = [ctypes.POINTER(Desc)] + [_vp] * 10
_lib.qpb_solve_box_shared.restype = ctypes.c_int
_lib.qpb_solve_box_shared_host.argtypes = [ctypes.POINTER(Desc)] + [_vp] * 9
_lib.qpb_solve_box_shared_host.restype = ctypes.c_int
_lib.qpb_solve_box_shared_backward.argtypes = [ctypes.POINTER(Desc)] + [_vp] * 10
_lib.qpb_solve_box_shared_backward.restype = ctypes.c_int
_lib.qpb_solve_box_shared_backward_host.argtypes = [ctypes.POINTER(Desc)] + [_vp] * 9
_lib.qpb_solve_box_shared_backward_host.restype = ctypes.c_int
_lib.qpb_solve_box_backward_dual.argtypes = [ctypes.POINTER(Desc), ctypes.c_int32] + [_vp] * 11
_lib.qpb_solve_box_backward_dual.restype = ctypes.c_int
_lib.qpb_solve_box_backward_dual_host.argtypes = [ctypes.POINTER(Desc), ctypes.c_int32] + [_vp] * 10
_lib.qpb_solve_box_backward_dual_host.restype = ctypes.c_int
_lib.qpb_solve_factored_backward_multi.argtypes = [ctypes.POINTER(Desc)] + [_vp] * 3 + [ctypes.c_int32] * 2 + [_vp] * 5
_lib.qpb_solve_factored_backward_multi.restype = ctypes.c_int
_lib.qpb_solve_factored_backward_multi_host.argtypes = ([ctypes.POINTER(Desc)] + [_vp] * 3 + [ctypes.c_int32] * 2
                                                        + [_vp] * 4)
_lib.qpb_solve_factored_backward_multi_host.restype = ctypes.c_int
_lib.qpb_solve_box_backward_multi.argtypes = ([ctypes.POINTER(Desc), ctypes.c_int32] + [_vp] * 3 + [ctypes.c_int32]
                                              + [_vp] * 6)
_lib.qpb_solve_box_backward_multi.restype = ctypes.c_int
_lib.qpb_solve_box_backward_multi_host.argtypes = ([ctypes.POINTER(Desc), ctypes.c_int32] + [_vp] * 3
                                                   + [ctypes.c_int32] + [_vp] * 5)
_lib.qpb_solve_box_backward_multi_host.restype = ctypes.c_int
_lib.qpb_factor_box_doubles.argtypes = [ctypes.c_int32]
_lib.qpb_factor_box_doubles.restype = ctypes.c_int64
_lib.qpb_factor_box.argtypes = [ctypes.c_int32] + [_vp] * 4
_lib.qpb_factor_box.restype = ctypes.c_int
_lib.qpb_factor_box_host.argtypes = [ctypes.c_int32] + [_vp] * 3
_lib.qpb_factor_box_host.restype = ctypes.c_int
_lib.qpb_solve_box_factored.argtypes = [ctypes.POINTER(Desc)] + [_vp] * 10
_lib.qpb_solve_box_factored.restype = ctypes.c_int
_lib.qpb_solve_box_factored_host.argtypes = [ctypes.POINTER(Desc)] + [_vp] * 9
_lib.qpb_solve_box_factored_host.restype = ctypes.c_int
_lib.qpb_ref_solve.argtypes = [ctypes.POINTER(RefDesc)] + [_vp] * 6
_lib.qpb_ref_solve.restype = ctypes.c_int
_lib.qpb_ref_solve_host.argtypes = [ctypes.POINTER(RefDesc)] + [_vp] * 5
_lib.qpb_ref_solve_host.restype = ctypes.c_int
_lib.qpb_qf_eval.argtypes = [ctypes.c_int32, ctypes.c_int64, _vp, _vp, ctypes.c_double, _vp, _vp, _vp]
_lib.qpb_qf_eval.restype = ctypes.c_int
_lib.qpb_matrix_invert.argtypes = [ctypes.c_int32, ctypes.c_int64, _vp, _vp, _vp]
_lib.qpb_matrix_invert.restype = ctypes.c_int
_lib.qpb_last_error.restype = ctypes.c_char_p
_lib.qpb_version.restype = ctypes.c_char_p
_lib.qpb_device_count.restype = ctypes.c_int
_lib.qpb_set_device.argtypes = [ctypes.c_int]
_lib.qpb_synchronize.argtypes = [_vp]


class QPBError(RuntimeError):
    def __init__(self, code: int, where: str):
        msg = _lib.qpb_last_error().decode(errors="replace")
        super().__init__(f"{where} failed with {code}: {msg}")
        self.code = code


def _check(rc: int, where: str) -> None:
    if rc != 0:
        raise QPBError(rc, where)


def lib() -> ctypes.CDLL:
    return _lib


def version() -> str:
    return _lib.qpb_version().decode()


def device_count() -> int:
    return int(_lib.qpb_device_count())


class Solution(NamedTuple):
    x: object       # (B, n) float64
    lam: object     # (B, m) float64
    active: object  # (B, ceil(m/32)) int32 (uint32 bit pattern)
    status: object  # (B,) int32
    iters: object   # (B,) int32


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else ctypes.c_void_p(0)


def _stream_ptr(stream):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def _empty_solution(B: int, n: int, m: int, dev) -> Solution:
    import torch
    return Solution(torch.empty((B, n), dtype=torch.float64, device=dev),
                    torch.empty((B, m), dtype=torch.float64, device=dev),
                    torch.empty((B, (m + 31) // 32), dtype=torch.int32, device=dev),
                    torch.empty((B,), dtype=torch.int32, device=dev),
                    torch.empty((B,), dtype=torch.int32, device=dev))


def _solve_shape(who: str, H, f, A, b):
    """The argument checks solve and solve_eq share: (B, n, m) of contiguous float64 CUDA tensors."""
    import torch
    if not (H.is_cuda and f.is_cuda):
        raise ValueError(f"{who} expects CUDA (HIP) tensors; use solve_host for numpy")
    B, n = f.shape
    m = 0 if A is None else A.shape[1]
    for t in (H, f) + ((A, b) if m else ()):
        if t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError("inputs must be contiguous float64")
    if H.shape != (B, n, n) or (m and (A.shape != (B, m, n) or b.shape != (B, m))):
        raise ValueError("shape mismatch")
    return B, n, m


def solve(H, f, A=None, b=None, *, max_iter: int = 0, feas_tol: float = 0.0, out: Solution | None = None,
          stream=None, flags: int = 0) -> Solution:
    """Batched min 1/2 x^T H x + f^T x s.t. A x <= b on the GPU (torch CUDA float64 tensors).

    H (B,n,n), f (B,n), A (B,m,n), b (B,m).  Asynchronous on ``stream``
    (default: torch's current stream; the n > 32 class caches a scratch buffer per
    stream: call ``release_stream_workspace(stream)`` before destroying a stream
    passed here).  A/b omitted -> unconstrained solve.
    ``flags``: QPB_FLAG_DIAG_* kernel variants (measurement only, qpb.h).
    """
    B, n, m = _solve_shape("qpb.solve", H, f, A, b)
    if out is None:
        out = _empty_solution(B, n, m, f.device)
    d = Desc(n, m, B, max_iter, flags, feas_tol)
    rc = _lib.qpb_solve(ctypes.byref(d), _ptr(H), _ptr(f), _ptr(A) if m else None, _ptr(b) if m else None,
                        _ptr(out.x), _ptr(out.lam), _ptr(out.active), _ptr(out.status), _ptr(out.iters),
                        _stream_ptr(stream))
    _check(rc, "qpb_solve")
    return out


def solve_eq(H, f, A, b, meq: int, *, max_iter: int = 0, feas_tol: float = 0.0, out: Solution | None = None,
             stream=None) -> Solution:
    """Batched min 1/2 x^T H x + f^T x s.t. A[:meq] x = b[:meq], A[meq:] x <= b[meq:]
    on the GPU (qpb_solve_eq; torch CUDA float64 tensors as for ``solve``).

    For ``solve_qp(P, q, G, h, A, b)`` pass the stacked ``[A; G]``, ``[b; h]``
    and ``meq = rows(A)``.  ``lam[:, :meq]`` has either sign.  meq > 0 needs
    n <= 32 and m <= 64; meq == 0 is ``solve``.
    """
    B, n, m = _solve_shape("qpb.solve_eq", H, f, A, b)
    if out is None:
        out = _empty_solution(B, n, m, f.device)
    d = Desc(n, m, B, max_iter, 0, feas_tol)
    rc = _lib.qpb_solve_eq(ctypes.byref(d), int(meq), _ptr(H), _ptr(f), _ptr(A) if m else None,
                           _ptr(b) if m else None, _ptr(out.x), _ptr(out.lam), _ptr(out.active), _ptr(out.status),
                           _ptr(out.iters), _stream_ptr(stream))
    _check(rc, "qpb_solve_eq")
    return out


def solve_box(H, f, lb=None, ub=None, *, max_iter: int = 0, feas_tol: float = 0.0, out: Solution | None = None,
              stream=None) -> Solution:
    """Batched min 1/2 x^T H x + f^T x s.t. lb <= x <= ub on the GPU (qpb_solve_box,
    n <= 128): the reference admm()'s box QP (qp_solvers.c:146-319), solved exactly.

    H (B,n,n), f (B,n), lb / ub (B,n) CUDA float64 tensors or None (absent
    bounds; +-inf entries likewise).  The Solution has m = 2n: lam[:, :n] and
    active bits 0..n-1 belong to the upper bounds, lam[:, n:] and bits n..2n-1
    to the lower bounds (the row order of A = [I; -I], b = [ub; -lb]).
    """
    import torch
    if not (H.is_cuda and f.is_cuda):
        raise ValueError("qpb.solve_box expects CUDA (HIP) tensors")
    B, n = f.shape
    for t in (H, f, lb, ub):
        if t is not None and (t.dtype != torch.float64 or not t.is_contiguous()):
            raise ValueError("inputs must be contiguous float64")
        if t is not None and t.device != f.device:
            raise ValueError("H, f, lb and ub must live on the same CUDA device")
    if H.shape != (B, n, n) or any(t is not None and t.shape != (B, n) for t in (lb, ub)):
        raise ValueError("shape mismatch")
    m = 2 * n
    if out is None:
        out = _empty_solution(B, n, m, f.device)
    d = Desc(n, m, B, max_iter, 0, feas_tol)
    rc = _lib.qpb_solve_box(ctypes.byref(d), _ptr(H), _ptr(f), _ptr(lb), _ptr(ub), _ptr(out.x), _ptr(out.lam),
                            _ptr(out.active), _ptr(out.status), _ptr(out.iters), _stream_ptr(stream))
    _check(rc, "qpb_solve_box")
    return out


def solve_raw(desc: Desc, ptrs, stream_ptr) -> int:
    """Direct C-ABI call with raw device pointers (H, f, A, b, x, lam, active, status, iters)."""
    return _lib.qpb_solve(ctypes.byref(desc), *[ctypes.c_void_p(p) for p in ptrs], ctypes.c_void_p(stream_ptr))


def solve_host(H, f, A=None, b=None, *, max_iter: int = 0, feas_tol: float = 0.0) -> Solution:
    """numpy in / numpy out (qpb_solve_host: H2D, solve, D2H)."""
    return _solve_host(None, H, f, A, b, max_iter, feas_tol)


def solve_eq_host(H, f, A, b, meq: int, *, max_iter: int = 0, feas_tol: float = 0.0) -> Solution:
    """numpy in / numpy out (qpb_solve_eq_host): ``solve_eq`` with host arrays."""
    return _solve_host(int(meq), H, f, A, b, max_iter, feas_tol)


def _solve_host(meq, H, f, A, b, max_iter, feas_tol) -> Solution:
    import numpy as np
    H = np.ascontiguousarray(H, dtype=np.float64)
    f = np.ascontiguousarray(f, dtype=np.float64)
    B, n = f.shape
    m = 0 if A is None else A.shape[1]
    if m:
        A = np.ascontiguousarray(A, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
    w = (m + 31) // 32
    x = np.zeros((B, n))
    lam = np.zeros((B, m))
    act = np.zeros((B, w), dtype=np.uint32)
    st = np.zeros(B, dtype=np.int32)
    it = np.zeros(B, dtype=np.int32)
    d = Desc(n, m, B, max_iter, 0, feas_tol)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None  # noqa: E731
    if meq is None:
        rc = _lib.qpb_solve_host(ctypes.byref(d), p(H), p(f), p(A), p(b), p(x), p(lam), p(act), p(st), p(it))
        _check(rc, "qpb_solve_host")
    else:
        rc = _lib.qpb_solve_eq_host(ctypes.byref(d), meq, p(H), p(f), p(A), p(b), p(x), p(lam), p(act), p(st), p(it))
        _check(rc, "qpb_solve_eq_host")
    return Solution(x, lam, act, st, it)


NEED_ALL = ("H", "f", "A", "b")


def _need_set(need) -> set:
    need = set(need)
    if not need or not need <= set(NEED_ALL):
        raise ValueError(f"need must be a non-empty subset of {NEED_ALL}")
    return need


def solve_backward(H, A, sol: Solution, gx, *, need=NEED_ALL, stream=None):
    """Gradients of a solve through its KKT system (qpb_solve_backward): given
    ``sol`` from ``solve`` / ``solve_eq`` on (H, f, A, b) and the cotangent
    ``gx = dl/dx`` (B, n), returns ``(gH, gf, gA, gb)`` = dl/dH (B,n,n), dl/df
    (B,n), dl/dA (B,m,n), dl/db (B,m) at fixed active set (qpb.h has the
    contract).  Entries left out of ``need`` come back as None and are neither
    computed nor stored; with A None (m = 0) gA and gb are None.  ``sol.status``
    may be None: every QP then counts as OK.  QPs whose status is not OK get
    zeros.  n <= 32 and m <= 64; torch CUDA float64 tensors as for ``solve``.
    """
    import torch
    B, n, m = _solve_shape("qpb.solve_backward", H, gx, A, None if A is None else sol.lam)
    need = _need_set(need)
    if not sol.x.is_cuda or sol.x.dtype != torch.float64 or not sol.x.is_contiguous() or sol.x.shape != (B, n):
        raise ValueError("sol.x must be a contiguous float64 CUDA tensor of shape (B, n)")
    if m and (not sol.active.is_contiguous() or sol.active.shape != (B, (m + 31) // 32)
              or sol.active.element_size() != 4):
        raise ValueError("sol.active must be a contiguous (B, ceil(m/32)) tensor of 32-bit words")
    if sol.status is not None and (sol.status.dtype != torch.int32 or not sol.status.is_contiguous()
                                   or sol.status.shape != (B,)):
        raise ValueError("sol.status must be a contiguous int32 tensor of shape (B,) or None")
    dev = gx.device
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)  # noqa: E731
    gH = new(B, n, n) if "H" in need else None
    gf = new(B, n) if "f" in need else None
    gA = new(B, m, n) if m and "A" in need else None
    gb = new(B, m) if m and "b" in need else None
    if gH is None and gf is None and gA is None and gb is None:
        return None, None, None, None  # m == 0 and only A / b wanted
    d = Desc(n, m, B, 0, 0, 0.0)
    rc = _lib.qpb_solve_backward(ctypes.byref(d), _ptr(H), _ptr(A) if m else None, _ptr(sol.x),
                                 _ptr(sol.lam) if m else None, _ptr(sol.active) if m else None, _ptr(sol.status),
                                 _ptr(gx), _ptr(gH), _ptr(gf), _ptr(gA), _ptr(gb), _stream_ptr(stream))
    _check(rc, "qpb_solve_backward")
    return gH, gf, gA, gb


def solve_backward_host(H, A, sol: Solution, gx, *, need=NEED_ALL):
    """numpy in / numpy out (qpb_solve_backward_host): ``solve_backward`` with host arrays."""
    import numpy as np
    need = _need_set(need)
    H = np.ascontiguousarray(H, dtype=np.float64)
    gx = np.ascontiguousarray(gx, dtype=np.float64)
    x = np.ascontiguousarray(sol.x, dtype=np.float64)
    B, n = gx.shape
    m = 0 if A is None else A.shape[1]
    lam = act = None
    if m:
        A = np.ascontiguousarray(A, dtype=np.float64)
        lam = np.ascontiguousarray(sol.lam, dtype=np.float64)
        act = np.ascontiguousarray(np.asarray(sol.active).astype(np.uint32))
    st = None if sol.status is None else np.ascontiguousarray(sol.status, dtype=np.int32)
    gH = np.zeros((B, n, n)) if "H" in need else None
    gf = np.zeros((B, n)) if "f" in need else None
    gA = np.zeros((B, m, n)) if m and "A" in need else None
    gb = np.zeros((B, m)) if m and "b" in need else None
    if gH is None and gf is None and gA is None and gb is None:
        return None, None, None, None
    d = Desc(n, m, B, 0, 0, 0.0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None  # noqa: E731
    rc = _lib.qpb_solve_backward_host(ctypes.byref(d), p(H), p(A), p(x), p(lam), p(act), p(st), p(gx), p(gH), p(gf),
                                      p(gA), p(gb))
    _check(rc, "qpb_solve_backward_host")
    return gH, gf, gA, gb


def _shared_shape(who: str, H, f, A, b):
    """(B, n, m, shared) of a call whose H and / or A may be 2-D, one matrix for
    the whole batch: contiguous float64 CUDA tensors on one device."""
    import torch
    if not (H.is_cuda and f.is_cuda):
        raise ValueError(f"{who} expects CUDA (HIP) tensors; use the _host form for numpy")
    B, n = f.shape
    m = 0 if A is None else A.shape[-2]
    for t in (H, f) + ((A, b) if m else ()):
        if t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError("inputs must be contiguous float64")
        if t.device != f.device:
            raise ValueError("the inputs must live on the same CUDA device")
    shared = (SHARED_H if H.dim() == 2 else 0) | (SHARED_A if m and A.dim() == 2 else 0)
    if tuple(H.shape) not in ((n, n), (B, n, n)) or (m and (tuple(A.shape) not in ((m, n), (B, m, n))
                                                            or tuple(b.shape) != (B, m))):
        raise ValueError("shape mismatch")
    return B, n, m, shared


def solve_shared(H, f, A=None, b=None, meq: int = 0, *, max_iter: int = 0, feas_tol: float = 0.0,
                 out: Solution | None = None, stream=None) -> Solution:
    """``solve_eq`` with one H and / or one A for the whole batch (qpb_solve_shared).

    A 2-D ``H`` (n, n) is shared by all B QPs and read from that one copy; a
    3-D ``H`` (B, n, n) is batched as in ``solve``.  The same holds for ``A``
    (m, n) or (B, m, n).  f (B, n) and b (B, m) are per QP.  Every output is
    bit for bit what ``solve_eq`` gives on expanded copies.  With a shared
    operand n <= 32 and m <= 64."""
    B, n, m, shared = _shared_shape("qpb.solve_shared", H, f, A, b)
    if out is None:
        out = _empty_solution(B, n, m, f.device)
    d = Desc(n, m, B, max_iter, 0, feas_tol)
    rc = _lib.qpb_solve_shared(ctypes.byref(d), int(meq), shared, _ptr(H), _ptr(f), _ptr(A) if m else None,
                               _ptr(b) if m else None, _ptr(out.x), _ptr(out.lam), _ptr(out.active),
                               _ptr(out.status), _ptr(out.iters), _stream_ptr(stream))
    _check(rc, "qpb_solve_shared")
    return out


def solve_shared_host(H, f, A=None, b=None, meq: int = 0, *, max_iter: int = 0, feas_tol: float = 0.0) -> Solution:
    """numpy in / numpy out (qpb_solve_shared_host): ``solve_shared`` with host arrays."""
    import numpy as np
    H = np.ascontiguousarray(H, dtype=np.float64)
    f = np.ascontiguousarray(f, dtype=np.float64)
    B, n = f.shape
    m = 0 if A is None else A.shape[-2]
    if m:
        A = np.ascontiguousarray(A, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
    shared = (SHARED_H if H.ndim == 2 else 0) | (SHARED_A if m and A.ndim == 2 else 0)
    if H.shape not in ((n, n), (B, n, n)) or (m and (A.shape not in ((m, n), (B, m, n)) or b.shape != (B, m))):
        raise ValueError("shape mismatch")
    x = np.zeros((B, n))
    lam = np.zeros((B, m))
    act = np.zeros((B, (m + 31) // 32), dtype=np.uint32)
    st = np.zeros(B, dtype=np.int32)
    it = np.zeros(B, dtype=np.int32)
    d = Desc(n, m, B, max_iter, 0, feas_tol)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None  # noqa: E731
    rc = _lib.qpb_solve_shared_host(ctypes.byref(d), int(meq), shared, p(H), p(f), p(A) if m else None,
                                    p(b) if m else None, p(x), p(lam), p(act), p(st), p(it))
    _check(rc, "qpb_solve_shared_host")
    return Solution(x, lam, act, st, it)


class SharedFactor(NamedTuple):
    """One shared H and A, factored once (qpb_factor_shared): the input of ``solve_factored``."""
    fac: object     # (factor_doubles(n, m),) float64: L, D = A L^-T, the rows' norms, A (layout internal)
    n: int
    m: int
    status: object  # (1,) int32: OK, NOT_SPD, or NUMERICAL for a NaN or overflowing row of A


def factor_doubles(n: int, m: int) -> int:
    """Doubles a factor buffer for (n, m) holds (qpb_factor_doubles; n <= 32, m <= 64)."""
    k = int(_lib.qpb_factor_doubles(int(n), int(m)))
    if k < 0:
        _check(k, "qpb_factor_doubles")
    return k


def factor_shared(H, A=None, *, stream=None) -> SharedFactor:
    """Factor ONE H (n, n) and ONE A (m, n) for a whole batch, once
    (qpb_factor_shared): torch CUDA float64 tensors, one small launch,
    asynchronous on ``stream``.  The result goes to ``solve_factored`` any
    number of times -- an MPC loop factors once per model and solves every tick.
    n <= 32 and m <= 64."""
    import torch
    if not H.is_cuda:
        raise ValueError("qpb.factor_shared expects CUDA (HIP) tensors; use factor_shared_host for numpy")
    m = 0 if A is None else A.shape[0]
    for t in (H,) + ((A,) if m else ()):
        if t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError("inputs must be contiguous float64")
        if t.device != H.device:
            raise ValueError("the inputs must live on the same CUDA device")
    n = H.shape[-1]
    if tuple(H.shape) != (n, n) or (m and tuple(A.shape) != (m, n)):
        raise ValueError("shape mismatch: H must be (n, n) and A (m, n)")
    fac = torch.empty((factor_doubles(n, m),), dtype=torch.float64, device=H.device)
    status = torch.empty((1,), dtype=torch.int32, device=H.device)
    rc = _lib.qpb_factor_shared(n, m, _ptr(H), _ptr(A) if m else None, _ptr(fac), _ptr(status), _stream_ptr(stream))
    _check(rc, "qpb_factor_shared")
    return SharedFactor(fac, n, m, status)


def solve_factored(F: SharedFactor, f, b=None, meq: int = 0, *, max_iter: int = 0, feas_tol: float = 0.0,
                   out: Solution | None = None, stream=None) -> Solution:
    """``solve_shared`` with a 2-D H and A, without the per-QP set-up
    (qpb_solve_factored): ``F`` is ``factor_shared(H, A)``, f (B, n) and b (B, m)
    are per QP.  The contract is ``solve_shared``'s except that x and lam may
    differ from it by rounding and ``iters`` need not be the same."""
    import torch
    if not (f.is_cuda and F.fac.is_cuda):
        raise ValueError("qpb.solve_factored expects CUDA (HIP) tensors; use solve_factored_host for numpy")
    n, m = int(F.n), int(F.m)
    for t in (f,) + ((b,) if m else ()):
        if t is None or t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError("inputs must be contiguous float64")
        if t.device != F.fac.device:
            raise ValueError("the inputs must live on the factor's CUDA device")
    if f.dim() != 2 or f.shape[1] != n or (m and tuple(b.shape) != (f.shape[0], m)) or (not m and b is not None
                                                                                        and b.numel()):
        raise ValueError(f"shape mismatch: the factor is for n={n}, m={m}")
    if F.fac.dtype != torch.float64 or tuple(F.fac.shape) != (factor_doubles(n, m),) or not F.fac.is_contiguous():
        raise ValueError(f"the factor buffer is not one for n={n}, m={m}")
    B = f.shape[0]
    if out is None:
        out = _empty_solution(B, n, m, f.device)
    d = Desc(n, m, B, max_iter, 0, feas_tol)
    rc = _lib.qpb_solve_factored(ctypes.byref(d), int(meq), _ptr(F.fac), _ptr(f), _ptr(b) if m else None,
                                 _ptr(out.x), _ptr(out.lam), _ptr(out.active), _ptr(out.status), _ptr(out.iters),
                                 _stream_ptr(stream))
    _check(rc, "qpb_solve_factored")
    return out


def factor_shared_host(H, A=None) -> SharedFactor:
    """numpy in / numpy out (qpb_factor_shared_host): ``factor_shared`` with host arrays."""
    import numpy as np
    H = np.ascontiguousarray(H, dtype=np.float64)
    m = 0 if A is None else A.shape[0]
    n = H.shape[-1]
    if m:
        A = np.ascontiguousarray(A, dtype=np.float64)
    if H.shape != (n, n) or (m and A.shape != (m, n)):
        raise ValueError("shape mismatch: H must be (n, n) and A (m, n)")
    fac = np.zeros(factor_doubles(n, m))
    st = np.zeros(1, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None  # noqa: E731
    rc = _lib.qpb_factor_shared_host(n, m, p(H), p(A) if m else None, p(fac), p(st))
    _check(rc, "qpb_factor_shared_host")
    return SharedFactor(fac, n, m, st)


def solve_factored_host(F: SharedFactor, f, b=None, meq: int = 0, *, max_iter: int = 0,
                        feas_tol: float = 0.0) -> Solution:
    """numpy in / numpy out (qpb_solve_factored_host): ``solve_factored`` with host arrays."""
    import numpy as np
    n, m = int(F.n), int(F.m)
    fac = np.ascontiguousarray(F.fac, dtype=np.float64)
    f = np.ascontiguousarray(f, dtype=np.float64)
    if m:
        b = np.ascontiguousarray(b, dtype=np.float64)
    B = f.shape[0]
    if f.shape != (B, n) or (m and b.shape != (B, m)) or fac.shape != (factor_doubles(n, m),):
        raise ValueError(f"shape mismatch: the factor is for n={n}, m={m}")
    x = np.zeros((B, n))
    lam = np.zeros((B, m))
    act = np.zeros((B, (m + 31) // 32), dtype=np.uint32)
    st = np.zeros(B, dtype=np.int32)
    it = np.zeros(B, dtype=np.int32)
    d = Desc(n, m, B, max_iter, 0, feas_tol)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None  # noqa: E731
    rc = _lib.qpb_solve_factored_host(ctypes.byref(d), int(meq), p(fac), p(f), p(b) if m else None, p(x), p(lam),
                                      p(act), p(st), p(it))
    _check(rc, "qpb_solve_factored_host")
    return Solution(x, lam, act, st, it)


class RangeSolution(NamedTuple):
    x: object       # (B, n) float64
    lam: object     # (B, m) float64, signed: >= 0 at the upper bound, <= 0 at the lower one
    active: object  # (B, ceil(m/32)) int32 (uint32 bit pattern): active on either side
    lower: object   # (B, ceil(m/32)) int32 (uint32 bit pattern): active at the lower bound
    status: object  # (B,) int32
    iters: object   # (B,) int32


def _empty_range_solution(B: int, n: int, m: int, dev) -> RangeSolution:
    import torch
    s = _empty_solution(B, n, m, dev)
    return RangeSolution(s.x, s.lam, s.active, torch.empty((B, (m + 31) // 32), dtype=torch.int32, device=dev),
                         s.status, s.iters)


def solve_range(H, f, A, bl, bu, meq: int = 0, *, max_iter: int = 0, feas_tol: float = 0.0,
                out: RangeSolution | None = None, stream=None) -> RangeSolution:
    """Batched min 1/2 x^T H x + f^T x s.t. A[:meq] x = bu[:meq], bl[meq:] <= A[meq:] x <= bu[meq:]
    on the GPU (qpb_solve_range; torch CUDA float64 tensors as for ``solve``).

    The constraint form of OSQP and qpOASES: ``l``, ``u`` are ``bl``, ``bu`` and
    ``y`` is ``lam`` with the same sign (H x + f + A^T lam = 0).  ``bl`` or
    ``bu`` may be None (no row has that side); NaN and +-inf entries are absent
    bounds.  A 2-D ``H`` (n, n) and / or ``A`` (m, n) is one matrix for the whole
    batch, as in ``solve_shared``.  ``sol.active`` with ``sol.lam`` is what
    ``solve_backward`` reads; ``sol.lower`` marks the rows active at ``bl``.
    n <= 32 and m <= 64."""
    import torch
    if bl is None and bu is None and A is not None:
        raise ValueError("qpb.solve_range needs at least one of bl and bu")
    some = bu if bu is not None else bl
    B, n, m, shared = _shared_shape("qpb.solve_range", H, f, A, some)
    for t in (bl, bu):
        if m and t is not None and (t.dtype != torch.float64 or not t.is_contiguous() or t.device != f.device
                                    or tuple(t.shape) != (B, m)):
            raise ValueError("bl and bu must be contiguous float64 (B, m) tensors on the inputs' device")
    if out is None:
        out = _empty_range_solution(B, n, m, f.device)
    d = Desc(n, m, B, max_iter, 0, feas_tol)
    rc = _lib.qpb_solve_range(ctypes.byref(d), int(meq), shared, _ptr(H), _ptr(f), _ptr(A) if m else None,
                              _ptr(bl) if m else None, _ptr(bu) if m else None, _ptr(out.x), _ptr(out.lam),
                              _ptr(out.active), _ptr(out.lower), _ptr(out.status), _ptr(out.iters),
                              _stream_ptr(stream))
    _check(rc, "qpb_solve_range")
    return out


def solve_range_host(H, f, A, bl, bu, meq: int = 0, *, max_iter: int = 0, feas_tol: float = 0.0) -> RangeSolution:
    """numpy in / numpy out (qpb_solve_range_host): ``solve_range`` with host arrays."""
    import numpy as np
    H = np.ascontiguousarray(H, dtype=np.float64)
    f = np.ascontiguousarray(f, dtype=np.float64)
    B, n = f.shape
    m = 0 if A is None else A.shape[-2]
    if m:
        A = np.ascontiguousarray(A, dtype=np.float64)
        bl = None if bl is None else np.ascontiguousarray(bl, dtype=np.float64)
        bu = None if bu is None else np.ascontiguousarray(bu, dtype=np.float64)
    shared = (SHARED_H if H.ndim == 2 else 0) | (SHARED_A if m and A.ndim == 2 else 0)
    if H.shape not in ((n, n), (B, n, n)) or (m and (A.shape not in ((m, n), (B, m, n))
                                                     or any(t is not None and t.shape != (B, m) for t in (bl, bu)))):
        raise ValueError("shape mismatch")
    w = (m + 31) // 32
    x = np.zeros((B, n))
    lam = np.zeros((B, m))
    act = np.zeros((B, w), dtype=np.uint32)
    low = np.zeros((B, w), dtype=np.uint32)
    st = np.zeros(B, dtype=np.int32)
    it = np.zeros(B, dtype=np.int32)
    d = Desc(n, m, B, max_iter, 0, feas_tol)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None  # noqa: E731
    rc = _lib.qpb_solve_range_host(ctypes.byref(d), int(meq), shared, p(H), p(f), p(A) if m else None,
                                   p(bl) if m else None, p(bu) if m else None, p(x), p(lam), p(act), p(low), p(st),
                                   p(it))
    _check(rc, "qpb_solve_range_host")
    return RangeSolution(x, lam, act, low, st, it)


def solve_range_box(H, f, G, bl, bu, lb=None, ub=None, meq: int = 0, *, max_iter: int = 0, feas_tol: float = 0.0,
                    out: RangeSolution | None = None, stream=None) -> RangeSolution:
    """Batched min 1/2 x^T H x + f^T x s.t. G[:meq] x = bu[:meq], bl[meq:] <= G[meq:] x <= bu[meq:],
    lb <= x <= ub on the GPU (qpb_solve_range_box): qpOASES's and OSQP's whole form.

    ``G`` is (B, mg, n), or (mg, n) for the whole batch, or None (mg = 0: a box
    alone); ``bl``, ``bu`` are (B, mg) and ``lb``, ``ub`` (B, n).  Any of the
    four may be None -- that side is absent everywhere -- but not all of them.
    Every output is, bit for bit, ``solve_range``'s on the materialised
    ``[G; I]``, ``[bl; lb]``, ``[bu; ub]``, which is never built: ``lam`` is
    (B, mg + n), the rows first and then variable j at mg + j (>= 0 at ``ub``,
    <= 0 at ``lb``), ``active`` and ``lower`` have ceil((mg + n) / 32) words.
    A 2-D ``H`` and / or ``G`` is one matrix for the batch, as in ``solve_range``.
    n <= 32 and mg + n <= 64."""
    import torch
    if bl is None and bu is None and lb is None and ub is None:
        raise ValueError("qpb.solve_range_box needs at least one of bl, bu, lb and ub")
    if not (H.is_cuda and f.is_cuda):
        raise ValueError("qpb.solve_range_box expects CUDA (HIP) tensors; use solve_range_box_host for numpy")
    B, n = f.shape
    mg = 0 if G is None else G.shape[-2]
    for t in (H, f, G, bl, bu, lb, ub):
        if t is not None and (t.dtype != torch.float64 or not t.is_contiguous() or t.device != f.device):
            raise ValueError("inputs must be contiguous float64 tensors on one CUDA device")
    shared = (SHARED_H if H.dim() == 2 else 0) | (SHARED_A if mg and G.dim() == 2 else 0)
    if (tuple(H.shape) not in ((n, n), (B, n, n)) or (mg and tuple(G.shape) not in ((mg, n), (B, mg, n)))
            or any(t is not None and tuple(t.shape) != (B, mg) for t in (bl, bu))
            or any(t is not None and tuple(t.shape) != (B, n) for t in (lb, ub))):
        raise ValueError("shape mismatch")
    if out is None:
        out = _empty_range_solution(B, n, mg + n, f.device)
    d = Desc(n, mg, B, max_iter, 0, feas_tol)
    opt = lambda t: _ptr(t) if t is not None and t.numel() else None  # noqa: E731
    rc = _lib.qpb_solve_range_box(ctypes.byref(d), int(meq), shared, _ptr(H), _ptr(f), opt(G), opt(bl), opt(bu),
                                  opt(lb), opt(ub), _ptr(out.x), _ptr(out.lam), _ptr(out.active), _ptr(out.lower),
                                  _ptr(out.status), _ptr(out.iters), _stream_ptr(stream))
    _check(rc, "qpb_solve_range_box")
    return out


def solve_range_box_host(H, f, G, bl, bu, lb=None, ub=None, meq: int = 0, *, max_iter: int = 0,
                         feas_tol: float = 0.0) -> RangeSolution:
    """numpy in / numpy out (qpb_solve_range_box_host): ``solve_range_box`` with host arrays."""
    import numpy as np
    c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
    H, f, G, bl, bu, lb, ub = (c(a) for a in (H, f, G, bl, bu, lb, ub))
    B, n = f.shape
    mg = 0 if G is None else G.shape[-2]
    shared = (SHARED_H if H.ndim == 2 else 0) | (SHARED_A if mg and G.ndim == 2 else 0)
    if (H.shape not in ((n, n), (B, n, n)) or (mg and G.shape not in ((mg, n), (B, mg, n)))
            or any(t is not None and t.shape != (B, mg) for t in (bl, bu))
            or any(t is not None and t.shape != (B, n) for t in (lb, ub))):
        raise ValueError("shape mismatch")
    m = mg + n
    w = (m + 31) // 32
    x = np.zeros((B, n))
    lam = np.zeros((B, m))
    act = np.zeros((B, w), dtype=np.uint32)
    low = np.zeros((B, w), dtype=np.uint32)
    st = np.zeros(B, dtype=np.int32)
    it = np.zeros(B, dtype=np.int32)
    d = Desc(n, mg, B, max_iter, 0, feas_tol)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None  # noqa: E731
    rc = _lib.qpb_solve_range_box_host(ctypes.byref(d), int(meq), shared, p(H), p(f), p(G), p(bl), p(bu), p(lb),
                                       p(ub), p(x), p(lam), p(act), p(low), p(st), p(it))
    _check(rc, "qpb_solve_range_box_host")
    return RangeSolution(x, lam, act, low, st, it)


RANGE_BOX_NEED_ALL = ("H", "f", "G", "bl", "bu", "lb", "ub")


def _range_box_need_set(need) -> set:
    need = set(need)
    if not need or not need <= set(RANGE_BOX_NEED_ALL):
        raise ValueError(f"need must be a non-empty subset of {RANGE_BOX_NEED_ALL}")
    return need


def solve_range_box_backward(H, G, sol: RangeSolution, gx, glam=None, *, need=RANGE_BOX_NEED_ALL, stream=None):
    """Gradients of ``solve_range_box`` through its KKT system
    (qpb_solve_range_box_backward), without ``[G; I]`` in memory: given ``sol``
    from that call on (H, f, G, bl, bu, lb, ub), the cotangent ``gx = dl/dx``
    (B, n) and, for a loss that reads the multipliers, ``glam = dl/dlam``
    (B, mg + n) in ``sol.lam``'s layout, returns ``(gH, gf, gG, gbl, gbu, glb,
    gub)``: gH and gG in the shapes of H and G (a 2-D one is shared and its
    gradient is ONE matrix, the sum over the batch), gf, glb, gub (B, n) and gbl,
    gbu (B, mg).  Every output is, bit for bit, ``solve_backward_dual`` on the
    materialised ``[G; I]`` -- gG its first mg rows, its gb routed by
    ``sol.lower``: to the lower bound's array where the row's bit is set, to the
    upper bound's otherwise, +0.0 in the other.  An entry is None where its name
    is not in ``need``, and gG at ``G is None``.  ``glam=None`` is the call
    without it, launch for launch.  n <= 32 and mg + n <= 64."""
    import torch
    need = _range_box_need_set(need)
    if not (H.is_cuda and gx.is_cuda):
        raise ValueError("qpb.solve_range_box_backward expects CUDA (HIP) tensors; use solve_range_box_backward_host")
    B, n = gx.shape
    mg = 0 if G is None else G.shape[-2]
    m = mg + n
    w = (m + 31) // 32
    for t in (H, G, gx, glam, sol.x, sol.lam):
        if t is not None and (t.dtype != torch.float64 or not t.is_contiguous() or t.device != gx.device):
            raise ValueError("inputs must be contiguous float64 tensors on one CUDA device")
    if (tuple(H.shape) not in ((n, n), (B, n, n)) or (mg and tuple(G.shape) not in ((mg, n), (B, mg, n)))
            or tuple(sol.x.shape) != (B, n) or tuple(sol.lam.shape) != (B, m)
            or (glam is not None and tuple(glam.shape) != (B, m))):
        raise ValueError("shape mismatch")
    for name, t in (("active", sol.active), ("lower", sol.lower)):
        if t is not None and (not t.is_contiguous() or tuple(t.shape) != (B, w) or t.element_size() != 4):
            raise ValueError(f"sol.{name} must be a contiguous (B, ceil((mg + n)/32)) tensor of 32-bit words")
    if sol.active is None:
        raise ValueError("sol.active is required")
    if sol.lower is None and ("bl" in need or "lb" in need):
        raise ValueError("sol.lower is required for the gradients of bl and lb")
    if sol.status is not None and (sol.status.dtype != torch.int32 or not sol.status.is_contiguous()
                                   or tuple(sol.status.shape) != (B,)):
        raise ValueError("sol.status must be a contiguous int32 tensor of shape (B,) or None")
    shared = (SHARED_H if H.dim() == 2 else 0) | (SHARED_A if mg and G.dim() == 2 else 0)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=gx.device)  # noqa: E731
    gH = new(*H.shape) if "H" in need else None
    gf = new(B, n) if "f" in need else None
    gG = new(*G.shape) if mg and "G" in need else None
    gbl = new(B, mg) if "bl" in need else None
    gbu = new(B, mg) if "bu" in need else None
    glb = new(B, n) if "lb" in need else None
    gub = new(B, n) if "ub" in need else None
    outs = (gH, gf, gG, gbl, gbu, glb, gub)
    if all(t is None or not t.numel() for t in outs):
        return outs  # mg == 0 and only G / bl / bu wanted
    opt = lambda t: _ptr(t) if t is not None and t.numel() else None  # noqa: E731
    d = Desc(n, mg, B, 0, 0, 0.0)
    rc = _lib.qpb_solve_range_box_backward(ctypes.byref(d), shared, _ptr(H), opt(G), _ptr(sol.x), _ptr(sol.lam),
                                           _ptr(sol.active), opt(sol.lower), opt(sol.status), _ptr(gx), opt(glam),
                                           opt(gH), opt(gf), opt(gG), opt(gbl), opt(gbu), opt(glb), opt(gub),
                                           _stream_ptr(stream))
    _check(rc, "qpb_solve_range_box_backward")
    return outs


def solve_range_box_backward_host(H, G, sol: RangeSolution, gx, glam=None, *, need=RANGE_BOX_NEED_ALL):
    """numpy in / numpy out (qpb_solve_range_box_backward_host): ``solve_range_box_backward`` with host arrays."""
    import numpy as np
    need = _range_box_need_set(need)
    c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
    H, G, gx, glam, x, lam = (c(a) for a in (H, G, gx, glam, sol.x, sol.lam))
    B, n = gx.shape
    mg = 0 if G is None else G.shape[-2]
    m = mg + n
    w = (m + 31) // 32
    u32 = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a).astype(np.uint32))  # noqa: E731
    act, low = u32(sol.active), u32(sol.lower)
    shared = (SHARED_H if H.ndim == 2 else 0) | (SHARED_A if mg and G.ndim == 2 else 0)
    if (H.shape not in ((n, n), (B, n, n)) or (mg and G.shape not in ((mg, n), (B, mg, n))) or x.shape != (B, n)
            or lam.shape != (B, m) or act is None or act.shape != (B, w) or (low is not None and low.shape != (B, w))
            or (glam is not None and glam.shape != (B, m))):
        raise ValueError("shape mismatch")
    if low is None and ("bl" in need or "lb" in need):
        raise ValueError("sol.lower is required for the gradients of bl and lb")
    st = None if sol.status is None else np.ascontiguousarray(sol.status, dtype=np.int32)
    gH = np.zeros(H.shape) if "H" in need else None
    gf = np.zeros((B, n)) if "f" in need else None
    gG = np.zeros(G.shape) if mg and "G" in need else None
    gbl = np.zeros((B, mg)) if "bl" in need else None
    gbu = np.zeros((B, mg)) if "bu" in need else None
    glb = np.zeros((B, n)) if "lb" in need else None
    gub = np.zeros((B, n)) if "ub" in need else None
    outs = (gH, gf, gG, gbl, gbu, glb, gub)
    if all(t is None or not t.size for t in outs):
        return outs
    d = Desc(n, mg, B, 0, 0, 0.0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None  # noqa: E731
    rc = _lib.qpb_solve_range_box_backward_host(ctypes.byref(d), shared, p(H), p(G), p(x), p(lam), p(act), p(low),
                                                p(st), p(gx), p(glam), p(gH), p(gf), p(gG), p(gbl), p(gbu), p(glb),
                                                p(gub))
    _check(rc, "qpb_solve_range_box_backward_host")
    return outs


def solve_range_factored(F: SharedFactor, f, bl, bu, meq: int = 0, *, max_iter: int = 0, feas_tol: float = 0.0,
                         out: RangeSolution | None = None, stream=None) -> RangeSolution:
    """``solve_range`` with a 2-D H and A, without the per-QP set-up
    (qpb_solve_range_factored): ``F`` is ``factor_shared(H, A)`` -- the buffer
    ``solve_factored`` takes, unchanged -- and f (B, n), bl and bu (B, m) are per
    QP; ``bl`` or ``bu`` may be None.  The contract is ``solve_range``'s except
    that x and lam may differ from it by rounding and ``iters`` need not be the
    same.  An MPC loop factors once per model and calls this every tick."""
    import torch
    if not (f.is_cuda and F.fac.is_cuda):
        raise ValueError("qpb.solve_range_factored expects CUDA (HIP) tensors; use solve_range_factored_host for numpy")
    n, m = int(F.n), int(F.m)
    if m and bl is None and bu is None:
        raise ValueError("qpb.solve_range_factored needs at least one of bl and bu")
    if f.dtype != torch.float64 or not f.is_contiguous() or f.device != F.fac.device:
        raise ValueError("f must be a contiguous float64 tensor on the factor's CUDA device")
    if f.dim() != 2 or f.shape[1] != n:
        raise ValueError(f"shape mismatch: the factor is for n={n}, m={m}")
    B = f.shape[0]
    for t in (bl, bu):
        if m and t is not None and (t.dtype != torch.float64 or not t.is_contiguous() or t.device != f.device
                                    or tuple(t.shape) != (B, m)):
            raise ValueError(f"bl and bu must be contiguous float64 (B, m) tensors on the factor's device: the "
                             f"factor is for n={n}, m={m}")
        if not m and t is not None and t.numel():
            raise ValueError(f"shape mismatch: the factor is for n={n}, m={m}")
    if F.fac.dtype != torch.float64 or tuple(F.fac.shape) != (factor_doubles(n, m),) or not F.fac.is_contiguous():
        raise ValueError(f"the factor buffer is not one for n={n}, m={m}")
    if out is None:
        out = _empty_range_solution(B, n, m, f.device)
    d = Desc(n, m, B, max_iter, 0, feas_tol)
    rc = _lib.qpb_solve_range_factored(ctypes.byref(d), int(meq), _ptr(F.fac), _ptr(f),
                                       _ptr(bl) if m and bl is not None else None,
                                       _ptr(bu) if m and bu is not None else None, _ptr(out.x), _ptr(out.lam),
                                       _ptr(out.active), _ptr(out.lower), _ptr(out.status), _ptr(out.iters),
                                       _stream_ptr(stream))
    _check(rc, "qpb_solve_range_factored")
    return out


def solve_range_factored_host(F: SharedFactor, f, bl, bu, meq: int = 0, *, max_iter: int = 0,
                              feas_tol: float = 0.0) -> RangeSolution:
    """numpy in / numpy out (qpb_solve_range_factored_host): ``solve_range_factored`` with host arrays."""
    import numpy as np
    n, m = int(F.n), int(F.m)
    fac = np.ascontiguousarray(F.fac, dtype=np.float64)
    f = np.ascontiguousarray(f, dtype=np.float64)
    if m:
        bl = None if bl is None else np.ascontiguousarray(bl, dtype=np.float64)
        bu = None if bu is None else np.ascontiguousarray(bu, dtype=np.float64)
    B = f.shape[0]
    if f.shape != (B, n) or fac.shape != (factor_doubles(n, m),) or (
            m and any(t is not None and t.shape != (B, m) for t in (bl, bu))):
        raise ValueError(f"shape mismatch: the factor is for n={n}, m={m}")
    w = (m + 31) // 32
    x = np.zeros((B, n))
    lam = np.zeros((B, m))
    act = np.zeros((B, w), dtype=np.uint32)
    low = np.zeros((B, w), dtype=np.uint32)
    st = np.zeros(B, dtype=np.int32)
    it = np.zeros(B, dtype=np.int32)
    d = Desc(n, m, B, max_iter, 0, feas_tol)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None  # noqa: E731
    rc = _lib.qpb_solve_range_factored_host(ctypes.byref(d), int(meq), p(fac), p(f), p(bl) if m else None,
                                            p(bu) if m else None, p(x), p(lam), p(act), p(low), p(st), p(it))
    _check(rc, "qpb_solve_range_factored_host")
    return RangeSolution(x, lam, act, low, st, it)


def solve_shared_backward(H, A, sol: Solution, gx, *, need=NEED_ALL, stream=None):
    """``solve_backward`` with one H and / or one A for the whole batch
    (qpb_solve_shared_backward): a 2-D ``H`` (n, n) or ``A`` (m, n) is shared, and
    its gradient comes back as ONE matrix of that shape, the sum over the batch
    (QPs whose status is not OK contribute exactly 0); no (B, n, n) or
    (B, m, n) tensor is allocated for it.  gf (B, n), gb (B, m) and the
    gradient of a 3-D operand are ``solve_backward``'s bit for bit.  The sums
    use the stream's cached workspace (``release_stream_workspace``).  With a
    shared operand n <= 32 and m <= 64."""
    import torch
    B, n, m, shared = _shared_shape("qpb.solve_shared_backward", H, gx, A, None if A is None else sol.lam)
    need = _need_set(need)
    if not sol.x.is_cuda or sol.x.dtype != torch.float64 or not sol.x.is_contiguous() or sol.x.shape != (B, n):
        raise ValueError("sol.x must be a contiguous float64 CUDA tensor of shape (B, n)")
    if m and (not sol.active.is_contiguous() or sol.active.shape != (B, (m + 31) // 32)
              or sol.active.element_size() != 4):
        raise ValueError("sol.active must be a contiguous (B, ceil(m/32)) tensor of 32-bit words")
    if sol.status is not None and (sol.status.dtype != torch.int32 or not sol.status.is_contiguous()
                                   or sol.status.shape != (B,)):
        raise ValueError("sol.status must be a contiguous int32 tensor of shape (B,) or None")
    dev = gx.device
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)  # noqa: E731
    gH = new(*H.shape) if "H" in need else None
    gf = new(B, n) if "f" in need else None
    gA = new(*A.shape) if m and "A" in need else None
    gb = new(B, m) if m and "b" in need else None
    if gH is None and gf is None and gA is None and gb is None:
        return None, None, None, None  # m == 0 and only A / b wanted
    d = Desc(n, m, B, 0, 0, 0.0)
    rc = _lib.qpb_solve_shared_backward(ctypes.byref(d), shared, _ptr(H), _ptr(A) if m else None, _ptr(sol.x),
                                        _ptr(sol.lam) if m else None, _ptr(sol.active) if m else None,
                                        _ptr(sol.status), _ptr(gx), _ptr(gH), _ptr(gf), _ptr(gA), _ptr(gb),
                                        _stream_ptr(stream))
    _check(rc, "qpb_solve_shared_backward")
    return gH, gf, gA, gb


def solve_shared_backward_host(H, A, sol: Solution, gx, *, need=NEED_ALL):
    """numpy in / numpy out (qpb_solve_shared_backward_host): ``solve_shared_backward`` with host arrays."""
    import numpy as np
    need = _need_set(need)
    H = np.ascontiguousarray(H, dtype=np.float64)
    gx = np.ascontiguousarray(gx, dtype=np.float64)
    x = np.ascontiguousarray(sol.x, dtype=np.float64)
    B, n = gx.shape
    m = 0 if A is None else A.shape[-2]
    lam = act = None
    if m:
        A = np.ascontiguousarray(A, dtype=np.float64)
        lam = np.ascontiguousarray(sol.lam, dtype=np.float64)
        act = np.ascontiguousarray(np.asarray(sol.active).astype(np.uint32))
    shared = (SHARED_H if H.ndim == 2 else 0) | (SHARED_A if m and A.ndim == 2 else 0)
    if H.shape not in ((n, n), (B, n, n)) or x.shape != (B, n) or (m and A.shape not in ((m, n), (B, m, n))):
        raise ValueError("shape mismatch")
    st = None if sol.status is None else np.ascontiguousarray(sol.status, dtype=np.int32)
    gH = np.zeros(H.shape) if "H" in need else None
    gf = np.zeros((B, n)) if "f" in need else None
    gA = np.zeros(A.shape) if m and "A" in need else None
    gb = np.zeros((B, m)) if m and "b" in need else None
    if gH is None and gf is None and gA is None and gb is None:
        return None, None, None, None
    d = Desc(n, m, B, 0, 0, 0.0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None  # noqa: E731
    rc = _lib.qpb_solve_shared_backward_host(ctypes.byref(d), shared, p(H), p(A), p(x), p(lam), p(act), p(st), p(gx),
                                             p(gH), p(gf), p(gA), p(gb))
    _check(rc, "qpb_solve_shared_backward_host")
    return gH, gf, gA, gb


def solve_backward_dual(H, A, sol: Solution, gx, glam, *, need=NEED_ALL, stream=None):
    """``solve_shared_backward`` for a loss that also reads the multipliers
    (qpb_solve_backward_dual): ``glam = dl/dlam`` (B, m), in ``sol.lam``'s layout
    and sign convention, is the lower right-hand side of the same KKT system,
    and (gH, gf, gA, gb) are ``solve_backward``'s formulas on its solution.
    A 2-D ``H`` or ``A`` is shared and its gradient is ONE matrix, the sum over
    the batch, as in ``solve_shared_backward``.  ``glam`` outside the active set
    and of QPs whose status is not OK is ignored, whatever it holds.
    ``glam=None`` (or m = 0) is ``solve_shared_backward(H, A, sol, gx)``, bit for
    bit.  n <= 32 and m <= 64."""
    import torch
    B, n, m, shared = _shared_shape("qpb.solve_backward_dual", H, gx, A, None if A is None else sol.lam)
    need = _need_set(need)
    if not sol.x.is_cuda or sol.x.dtype != torch.float64 or not sol.x.is_contiguous() or sol.x.shape != (B, n):
        raise ValueError("sol.x must be a contiguous float64 CUDA tensor of shape (B, n)")
    if m and (not sol.active.is_contiguous() or sol.active.shape != (B, (m + 31) // 32)
              or sol.active.element_size() != 4):
        raise ValueError("sol.active must be a contiguous (B, ceil(m/32)) tensor of 32-bit words")
    if sol.status is not None and (sol.status.dtype != torch.int32 or not sol.status.is_contiguous()
                                   or sol.status.shape != (B,)):
        raise ValueError("sol.status must be a contiguous int32 tensor of shape (B,) or None")
    if glam is not None and (not glam.is_cuda or glam.dtype != torch.float64 or not glam.is_contiguous()
                             or glam.device != gx.device or tuple(glam.shape) != (B, m)):
        raise ValueError("glam must be a contiguous float64 CUDA tensor of shape (B, m) on gx's device, or None")
    dev = gx.device
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)  # noqa: E731
    gH = new(*H.shape) if "H" in need else None
    gf = new(B, n) if "f" in need else None
    gA = new(*A.shape) if m and "A" in need else None
    gb = new(B, m) if m and "b" in need else None
    if gH is None and gf is None and gA is None and gb is None:
        return None, None, None, None  # m == 0 and only A / b wanted
    d = Desc(n, m, B, 0, 0, 0.0)
    rc = _lib.qpb_solve_backward_dual(ctypes.byref(d), shared, _ptr(H), _ptr(A) if m else None, _ptr(sol.x),
                                      _ptr(sol.lam) if m else None, _ptr(sol.active) if m else None,
                                      _ptr(sol.status), _ptr(gx), _ptr(glam) if m else None, _ptr(gH), _ptr(gf),
                                      _ptr(gA), _ptr(gb), _stream_ptr(stream))
    _check(rc, "qpb_solve_backward_dual")
    return gH, gf, gA, gb


def solve_backward_dual_host(H, A, sol: Solution, gx, glam, *, need=NEED_ALL):
    """numpy in / numpy out (qpb_solve_backward_dual_host): ``solve_backward_dual`` with host arrays."""
    import numpy as np
    need = _need_set(need)
    H = np.ascontiguousarray(H, dtype=np.float64)
    gx = np.ascontiguousarray(gx, dtype=np.float64)
    x = np.ascontiguousarray(sol.x, dtype=np.float64)
    B, n = gx.shape
    m = 0 if A is None else A.shape[-2]
    lam = act = None
    if m:
        A = np.ascontiguousarray(A, dtype=np.float64)
        lam = np.ascontiguousarray(sol.lam, dtype=np.float64)
        act = np.ascontiguousarray(np.asarray(sol.active).astype(np.uint32))
    glam = None if glam is None or not m else np.ascontiguousarray(glam, dtype=np.float64)
    shared = (SHARED_H if H.ndim == 2 else 0) | (SHARED_A if m and A.ndim == 2 else 0)
    if H.shape not in ((n, n), (B, n, n)) or x.shape != (B, n) or (m and A.shape not in ((m, n), (B, m, n))) or (
            glam is not None and glam.shape != (B, m)):
        raise ValueError("shape mismatch")
    st = None if sol.status is None else np.ascontiguousarray(sol.status, dtype=np.int32)
    gH = np.zeros(H.shape) if "H" in need else None
    gf = np.zeros((B, n)) if "f" in need else None
    gA = np.zeros(A.shape) if m and "A" in need else None
    gb = np.zeros((B, m)) if m and "b" in need else None
    if gH is None and gf is None and gA is None and gb is None:
        return None, None, None, None
    d = Desc(n, m, B, 0, 0, 0.0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None  # noqa: E731
    rc = _lib.qpb_solve_backward_dual_host(ctypes.byref(d), shared, p(H), p(A), p(x), p(lam), p(act), p(st), p(gx),
                                           p(glam), p(gH), p(gf), p(gA), p(gb))
    _check(rc, "qpb_solve_backward_dual_host")
    return gH, gf, gA, gb


def solve_tangent(H, A, sol: Solution, df, db=None, *, stream=None):
    """The forward sensitivity of a solve: the tangent ``(dx, dlam)`` of
    (x*, lam*) along a change ``df`` (B, n) of f and ``db`` (B, m) of b, at fixed
    active set.  Differentiating H x + f + A_W^T lam = 0, A_W x = b_W gives
    K [dx; dlam_W] = -[df; -db_W] with the KKT matrix K of ``solve_backward``,
    which is symmetric: the tangent is ONE call of ``solve_backward_dual`` with
    ``gx = df``, ``glam = -db`` and ``need = ("f", "b")``, and
    ``(dx, dlam) = (gf, -gb)``.  ``dlam`` is 0 outside the active set, and both
    are 0 for a QP whose status is not OK.  ``db=None`` is db = 0 and runs
    ``solve_backward``'s kernels.  With A None (m = 0) ``dlam`` is None.  For an
    MPC law u*(x0), with f and b affine in the state x0, this is the local
    affine law u* + K (x0 - x0*) one column at a time."""
    import contextlib

    import torch
    m = 0 if A is None else A.shape[-2]
    # (the two negations run on the call's stream as well)
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        glam = None if db is None or not m else -db
        _, dx, _, gb = solve_backward_dual(H, A, sol, df, glam, need=("f", "b"), stream=stream)
        return dx, (None if gb is None else -gb)


class BackwardFactor(NamedTuple):
    """One shared H and A, factored once for the backward (qpb_factor_shared_backward):
    the input of ``solve_factored_backward``.  Not a ``SharedFactor``: the buffer
    is the backward kernels' own."""
    fac: object     # (factor_backward_doubles(n, m),) float64: L, 1 / L_kk, D = A L^-T, the multipliers (layout internal)
    n: int
    m: int
    status: object  # (1,) int32: OK or NOT_SPD


def factor_backward_doubles(n: int, m: int) -> int:
    """Doubles a backward factor buffer for (n, m) holds (qpb_factor_backward_doubles; n <= 32, m <= 64)."""
    k = int(_lib.qpb_factor_backward_doubles(int(n), int(m)))
    if k < 0:
        _check(k, "qpb_factor_backward_doubles")
    return k


def factor_shared_backward(H, A=None, *, stream=None) -> BackwardFactor:
    """Factor ONE H (n, n) and ONE A (m, n) for the backward of a whole batch,
    once (qpb_factor_shared_backward): torch CUDA float64 tensors, one small
    launch, asynchronous on ``stream``.  The result goes to
    ``solve_factored_backward`` any number of times.  n <= 32 and m <= 64."""
    import torch
    if not H.is_cuda:
        raise ValueError("qpb.factor_shared_backward expects CUDA (HIP) tensors; use factor_shared_backward_host "
                         "for numpy")
    m = 0 if A is None else A.shape[0]
    for t in (H,) + ((A,) if m else ()):
        if t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError("inputs must be contiguous float64")
        if t.device != H.device:
            raise ValueError("the inputs must live on the same CUDA device")
    n = H.shape[-1]
    if tuple(H.shape) != (n, n) or (m and tuple(A.shape) != (m, n)):
        raise ValueError("shape mismatch: H must be (n, n) and A (m, n)")
    fac = torch.empty((factor_backward_doubles(n, m),), dtype=torch.float64, device=H.device)
    status = torch.empty((1,), dtype=torch.int32, device=H.device)
    rc = _lib.qpb_factor_shared_backward(n, m, _ptr(H), _ptr(A) if m else None, _ptr(fac), _ptr(status),
                                         _stream_ptr(stream))
    _check(rc, "qpb_factor_shared_backward")
    return BackwardFactor(fac, n, m, status)


def solve_factored_backward(F: BackwardFactor, sol: Solution, gx, *, need=NEED_ALL, stream=None):
    """``solve_shared_backward`` with a 2-D H and A, without the per-QP set-up
    and without H and A (qpb_solve_factored_backward): ``F`` is
    ``factor_shared_backward(H, A)``.  Returns (gH (n, n), gf (B, n), gA (m, n),
    gb (B, m)), each bit for bit what ``solve_shared_backward(H, A, sol, gx)``
    returns; an entry is None where ``need`` leaves it out, and gA and gb with
    m == 0."""
    return _solve_factored_backward("solve_factored_backward", F, sol, gx, None, need, stream)


def solve_factored_backward_dual(F: BackwardFactor, sol: Solution, gx, glam, *, need=NEED_ALL, stream=None):
    """``solve_backward_dual`` with a 2-D H and A on a backward factor buffer
    (qpb_solve_factored_backward_dual): ``solve_factored_backward`` for a loss
    that also reads the multipliers, ``glam = dl/dlam`` (B, m) in ``sol.lam``'s
    layout and sign convention.  Every output is bit for bit what
    ``solve_backward_dual(H, A, sol, gx, glam)`` returns for the 2-D H and A that
    ``F`` was made from.  ``glam=None`` (or m = 0) is ``solve_factored_backward``,
    bit for bit."""
    return _solve_factored_backward("solve_factored_backward_dual", F, sol, gx, glam, need, stream)


def _solve_factored_backward(who: str, F: BackwardFactor, sol: Solution, gx, glam, need, stream):
    import torch
    if not (gx.is_cuda and F.fac.is_cuda):
        raise ValueError(f"qpb.{who} expects CUDA (HIP) tensors; use {who}_host "
                         "for numpy")
    n, m = int(F.n), int(F.m)
    need = _need_set(need)
    if gx.dtype != torch.float64 or not gx.is_contiguous():
        raise ValueError("inputs must be contiguous float64")
    if gx.dim() != 2 or gx.shape[1] != n:
        raise ValueError(f"shape mismatch: the factor is for n={n}, m={m}")
    B = gx.shape[0]
    if F.fac.dtype != torch.float64 or tuple(F.fac.shape) != (factor_backward_doubles(n, m),) \
            or not F.fac.is_contiguous():
        raise ValueError(f"the backward factor buffer is not one for n={n}, m={m}")
    if sol.x.device != gx.device or F.fac.device != gx.device:
        raise ValueError("the inputs must live on the factor's CUDA device")
    if not sol.x.is_cuda or sol.x.dtype != torch.float64 or not sol.x.is_contiguous() or sol.x.shape != (B, n):
        raise ValueError("sol.x must be a contiguous float64 CUDA tensor of shape (B, n)")
    if m and (sol.lam is None or sol.lam.dtype != torch.float64 or not sol.lam.is_contiguous()
              or sol.lam.shape != (B, m)):
        raise ValueError("sol.lam must be a contiguous float64 tensor of shape (B, m)")
    if m and (not sol.active.is_contiguous() or sol.active.shape != (B, (m + 31) // 32)
              or sol.active.element_size() != 4):
        raise ValueError("sol.active must be a contiguous (B, ceil(m/32)) tensor of 32-bit words")
    if sol.status is not None and (sol.status.dtype != torch.int32 or not sol.status.is_contiguous()
                                   or sol.status.shape != (B,)):
        raise ValueError("sol.status must be a contiguous int32 tensor of shape (B,) or None")
    if glam is not None and (not glam.is_cuda or glam.dtype != torch.float64 or not glam.is_contiguous()
                             or glam.device != gx.device or tuple(glam.shape) != (B, m)):
        raise ValueError("glam must be a contiguous float64 CUDA tensor of shape (B, m) on gx's device, or None")
    dev = gx.device
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)  # noqa: E731
    gH = new(n, n) if "H" in need else None
    gf = new(B, n) if "f" in need else None
    gA = new(m, n) if m and "A" in need else None
    gb = new(B, m) if m and "b" in need else None
    if gH is None and gf is None and gA is None and gb is None:
        return None, None, None, None  # m == 0 and only A / b wanted
    d = Desc(n, m, B, 0, 0, 0.0)
    if glam is None or not m:
        rc = _lib.qpb_solve_factored_backward(ctypes.byref(d), _ptr(F.fac), _ptr(sol.x), _ptr(sol.lam) if m else None,
                                              _ptr(sol.active) if m else None, _ptr(sol.status), _ptr(gx), _ptr(gH),
                                              _ptr(gf), _ptr(gA), _ptr(gb), _stream_ptr(stream))
        _check(rc, "qpb_solve_factored_backward")
    else:
        rc = _lib.qpb_solve_factored_backward_dual(ctypes.byref(d), _ptr(F.fac), _ptr(sol.x), _ptr(sol.lam),
                                                   _ptr(sol.active), _ptr(sol.status), _ptr(gx), _ptr(glam), _ptr(gH),
                                                   _ptr(gf), _ptr(gA), _ptr(gb), _stream_ptr(stream))
        _check(rc, "qpb_solve_factored_backward_dual")
    return gH, gf, gA, gb


def solve_factored_tangent(F: BackwardFactor, sol: Solution, df, db=None, *, stream=None):
    """``solve_tangent`` on a backward factor buffer: the tangent ``(dx, dlam)``
    of (x*, lam*) along ``df`` (B, n) and ``db`` (B, m) at fixed active set,
    without H and A and without the per-QP set-up -- ONE call of
    ``solve_factored_backward_dual`` with ``gx = df``, ``glam = -db`` and
    ``need = ("f", "b")``.  Bit for bit ``solve_tangent(H, A, sol, df, db)`` on
    the 2-D H and A that ``F`` was made from.  For an MPC loop that factors its
    plant model once, this is the local affine law around a tick's solution at
    the factored path's cost."""
    import contextlib

    import torch
    m = int(F.m)
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        glam = None if db is None or not m else -db
        _, dx, _, gb = solve_factored_backward_dual(F, sol, df, glam, need=("f", "b"), stream=stream)
        return dx, (None if gb is None else -gb)


def factor_shared_backward_host(H, A=None) -> BackwardFactor:
    """numpy in / numpy out (qpb_factor_shared_backward_host): ``factor_shared_backward`` with host arrays."""
    import numpy as np
    H = np.ascontiguousarray(H, dtype=np.float64)
    m = 0 if A is None else A.shape[0]
    n = H.shape[-1]
    if m:
        A = np.ascontiguousarray(A, dtype=np.float64)
    if H.shape != (n, n) or (m and A.shape != (m, n)):
        raise ValueError("shape mismatch: H must be (n, n) and A (m, n)")
    fac = np.zeros(factor_backward_doubles(n, m))
    st = np.zeros(1, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None  # noqa: E731
    rc = _lib.qpb_factor_shared_backward_host(n, m, p(H), p(A) if m else None, p(fac), p(st))
    _check(rc, "qpb_factor_shared_backward_host")
    return BackwardFactor(fac, n, m, st)


def solve_factored_backward_host(F: BackwardFactor, sol: Solution, gx, *, need=NEED_ALL):
    """numpy in / numpy out (qpb_solve_factored_backward_host): ``solve_factored_backward`` with host arrays."""
    return _solve_factored_backward_host(F, sol, gx, None, need)


def solve_factored_backward_dual_host(F: BackwardFactor, sol: Solution, gx, glam, *, need=NEED_ALL):
    """numpy in / numpy out (qpb_solve_factored_backward_dual_host): ``solve_factored_backward_dual`` with host
    arrays."""
    return _solve_factored_backward_host(F, sol, gx, glam, need)


def _solve_factored_backward_host(F: BackwardFactor, sol: Solution, gx, glam, need):
    import numpy as np
    need = _need_set(need)
    n, m = int(F.n), int(F.m)
    fac = np.ascontiguousarray(F.fac, dtype=np.float64)
    gx = np.ascontiguousarray(gx, dtype=np.float64)
    x = np.ascontiguousarray(sol.x, dtype=np.float64)
    B = gx.shape[0]
    lam = act = None
    if m:
        lam = np.ascontiguousarray(sol.lam, dtype=np.float64)
        act = np.ascontiguousarray(np.asarray(sol.active).astype(np.uint32))
    if gx.shape != (B, n) or x.shape != (B, n) or fac.shape != (factor_backward_doubles(n, m),) \
            or (m and (lam.shape != (B, m) or act.shape != (B, (m + 31) // 32))):
        raise ValueError(f"shape mismatch: the factor is for n={n}, m={m}")
    glam = None if glam is None or not m else np.ascontiguousarray(glam, dtype=np.float64)
    if glam is not None and glam.shape != (B, m):
        raise ValueError(f"shape mismatch: the factor is for n={n}, m={m}")
    st = None if sol.status is None else np.ascontiguousarray(sol.status, dtype=np.int32)
    gH = np.zeros((n, n)) if "H" in need else None
    gf = np.zeros((B, n)) if "f" in need else None
    gA = np.zeros((m, n)) if m and "A" in need else None
    gb = np.zeros((B, m)) if m and "b" in need else None
    if gH is None and gf is None and gA is None and gb is None:
        return None, None, None, None
    d = Desc(n, m, B, 0, 0, 0.0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None  # noqa: E731
    if glam is None:
        rc = _lib.qpb_solve_factored_backward_host(ctypes.byref(d), p(fac), p(x), p(lam), p(act), p(st), p(gx), p(gH),
                                                   p(gf), p(gA), p(gb))
        _check(rc, "qpb_solve_factored_backward_host")
    else:
        rc = _lib.qpb_solve_factored_backward_dual_host(ctypes.byref(d), p(fac), p(x), p(lam), p(act), p(st), p(gx),
                                                        p(glam), p(gH), p(gf), p(gA), p(gb))
        _check(rc, "qpb_solve_factored_backward_dual_host")
    return gH, gf, gA, gb


def sum_plan(batch: int):
    """(slots, QPs per slot) of the batch sum of ``solve_shared_backward``: the
    slice plan of csrc/qpb_route.h (qpb::sum_plan), a function of the batch size
    alone; tests/test_shared_plan.py holds the two together."""
    if batch <= 0:
        return 0, 0
    per = max((batch + SUM_MAX_SLOTS - 1) // SUM_MAX_SLOTS, SUM_MIN_SLICE)
    per = (per + 3) // 4 * 4
    return (batch + per - 1) // per, per


SUM_MAX_SLOTS, SUM_MIN_SLICE = 1024, 128  # kSumMaxSlots, kSumMinSlice

BOX_NEED_ALL = ("H", "f", "lb", "ub")


def _box_need_set(need) -> set:
    need = set(need)
    if not need or not need <= set(BOX_NEED_ALL):
        raise ValueError(f"need must be a non-empty subset of {BOX_NEED_ALL}")
    return need


def solve_box_backward(H, sol: Solution, gx, *, need=BOX_NEED_ALL, stream=None):
    """Gradients of a box solve (qpb_solve_box_backward): given ``sol`` from
    ``solve_box`` on (H, f, lb, ub) and the cotangent ``gx = dl/dx`` (B, n),
    returns ``(gH, gf, glb, gub)`` = dl/dH (B,n,n), dl/df, dl/dlb, dl/dub (B,n)
    at fixed active set (qpb.h has the contract).  Only ``sol.x``,
    ``sol.active`` and ``sol.status`` are read.  Entries left out of ``need``
    come back as None and are neither computed nor stored.  ``sol.status`` may
    be None: every QP then counts as OK.  QPs whose status is not OK get zeros.
    n <= 32; torch CUDA float64 tensors as for ``solve_box``.
    """
    import torch
    if not (H.is_cuda and gx.is_cuda):
        raise ValueError("qpb.solve_box_backward expects CUDA (HIP) tensors; use solve_box_backward_host for numpy")
    B, n = gx.shape
    for t in (H, gx):
        if t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError("inputs must be contiguous float64")
    if H.shape != (B, n, n):
        raise ValueError("shape mismatch")
    need = _box_need_set(need)
    if not sol.x.is_cuda or sol.x.dtype != torch.float64 or not sol.x.is_contiguous() or sol.x.shape != (B, n):
        raise ValueError("sol.x must be a contiguous float64 CUDA tensor of shape (B, n)")
    if (sol.active is None or not sol.active.is_cuda or not sol.active.is_contiguous()
            or sol.active.shape != (B, (2 * n + 31) // 32) or sol.active.element_size() != 4):
        raise ValueError("sol.active must be a contiguous (B, ceil(2n/32)) CUDA tensor of 32-bit words")
    if sol.status is not None and (sol.status.dtype != torch.int32 or not sol.status.is_contiguous()
                                   or sol.status.shape != (B,)):
        raise ValueError("sol.status must be a contiguous int32 tensor of shape (B,) or None")
    dev = gx.device
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)  # noqa: E731
    gH = new(B, n, n) if "H" in need else None
    gf = new(B, n) if "f" in need else None
    glb = new(B, n) if "lb" in need else None
    gub = new(B, n) if "ub" in need else None
    d = Desc(n, 2 * n, B, 0, 0, 0.0)
    rc = _lib.qpb_solve_box_backward(ctypes.byref(d), _ptr(H), _ptr(sol.x), _ptr(sol.active), _ptr(sol.status),
                                     _ptr(gx), _ptr(gH), _ptr(gf), _ptr(glb), _ptr(gub), _stream_ptr(stream))
    _check(rc, "qpb_solve_box_backward")
    return gH, gf, glb, gub


def solve_box_backward_host(H, sol: Solution, gx, *, need=BOX_NEED_ALL):
    """numpy in / numpy out (qpb_solve_box_backward_host): ``solve_box_backward`` with host arrays."""
    import numpy as np
    need = _box_need_set(need)
    H = np.ascontiguousarray(H, dtype=np.float64)
    gx = np.ascontiguousarray(gx, dtype=np.float64)
    x = np.ascontiguousarray(sol.x, dtype=np.float64)
    B, n = gx.shape
    act = np.ascontiguousarray(np.asarray(sol.active).astype(np.uint32))
    if H.shape != (B, n, n) or x.shape != (B, n) or act.shape != (B, (2 * n + 31) // 32):
        raise ValueError("shape mismatch")
    st = None if sol.status is None else np.ascontiguousarray(sol.status, dtype=np.int32)
    gH = np.zeros((B, n, n)) if "H" in need else None
    gf = np.zeros((B, n)) if "f" in need else None
    glb = np.zeros((B, n)) if "lb" in need else None
    gub = np.zeros((B, n)) if "ub" in need else None
    d = Desc(n, 2 * n, B, 0, 0, 0.0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None  # noqa: E731
    rc = _lib.qpb_solve_box_backward_host(ctypes.byref(d), p(H), p(x), p(act), p(st), p(gx), p(gH), p(gf), p(glb),
                                          p(gub))
    _check(rc, "qpb_solve_box_backward_host")
    return gH, gf, glb, gub


def solve_box_shared(H, f, lb=None, ub=None, *, max_iter: int = 0, feas_tol: float = 0.0,
                     out: Solution | None = None, stream=None) -> Solution:
    """``solve_box`` with ONE H (n, n) for the whole batch (qpb_solve_box_shared,
    n <= 128): H is read from one copy, no (B, n, n) tensor exists.  f (B,n),
    lb / ub (B,n) or None as for ``solve_box``; the Solution is, bit for bit,
    ``solve_box``'s on B copies of H.
    """
    import torch
    if not (H.is_cuda and f.is_cuda):
        raise ValueError("qpb.solve_box_shared expects CUDA (HIP) tensors; use solve_box_shared_host for numpy")
    B, n = f.shape
    for t in (H, f, lb, ub):
        if t is not None and (t.dtype != torch.float64 or not t.is_contiguous()):
            raise ValueError("inputs must be contiguous float64")
        if t is not None and t.device != f.device:
            raise ValueError("H, f, lb and ub must live on the same CUDA device")
    if H.shape != (n, n) or any(t is not None and t.shape != (B, n) for t in (lb, ub)):
        raise ValueError("shape mismatch: H must be (n, n), lb and ub (B, n)")
    m = 2 * n
    if out is None:
        out = _empty_solution(B, n, m, f.device)
    d = Desc(n, m, B, max_iter, 0, feas_tol)
    rc = _lib.qpb_solve_box_shared(ctypes.byref(d), _ptr(H), _ptr(f), _ptr(lb), _ptr(ub), _ptr(out.x),
                                   _ptr(out.lam), _ptr(out.active), _ptr(out.status), _ptr(out.iters),
                                   _stream_ptr(stream))
    _check(rc, "qpb_solve_box_shared")
    return out


def solve_box_shared_host(H, f, lb=None, ub=None, *, max_iter: int = 0, feas_tol: float = 0.0) -> Solution:
    """numpy in / numpy out (qpb_solve_box_shared_host): ``solve_box_shared`` with host arrays."""
    import numpy as np
    H = np.ascontiguousarray(H, dtype=np.float64)
    f = np.ascontiguousarray(f, dtype=np.float64)
    lb = None if lb is None else np.ascontiguousarray(lb, dtype=np.float64)
    ub = None if ub is None else np.ascontiguousarray(ub, dtype=np.float64)
    B, n = f.shape
    if H.shape != (n, n) or any(t is not None and t.shape != (B, n) for t in (lb, ub)):
        raise ValueError("shape mismatch: H must be (n, n), lb and ub (B, n)")
    m = 2 * n
    x = np.zeros((B, n))
    lam = np.zeros((B, m))
    act = np.zeros((B, (m + 31) // 32), dtype=np.uint32)
    st = np.zeros(B, dtype=np.int32)
    it = np.zeros(B, dtype=np.int32)
    d = Desc(n, m, B, max_iter, 0, feas_tol)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None  # noqa: E731
    rc = _lib.qpb_solve_box_shared_host(ctypes.byref(d), p(H), p(f), p(lb), p(ub), p(x), p(lam), p(act), p(st), p(it))
    _check(rc, "qpb_solve_box_shared_host")
    return Solution(x, lam, act, st, it)


class BoxFactor(NamedTuple):
    """One shared H of a batch of box QPs, factored once (qpb_factor_box): the input of ``solve_box_factored``."""
    fac: object     # (factor_box_doubles(n),) float64: L, the rows of L^-T and their squared norms (layout internal)
    n: int
    status: object  # (1,) int32: OK or NOT_SPD


def factor_box_doubles(n: int) -> int:
    """Doubles a box factor buffer for n holds (qpb_factor_box_doubles; n <= 32)."""
    k = int(_lib.qpb_factor_box_doubles(int(n)))
    if k < 0:
        _check(k, "qpb_factor_box_doubles")
    return k


def factor_box(H, *, stream=None) -> BoxFactor:
    """Factor ONE H (n, n) for a whole batch of box QPs, once (qpb_factor_box): a
    torch CUDA float64 tensor, one small launch, asynchronous on ``stream``.  The
    result goes to ``solve_box_factored`` any number of times.  n <= 32."""
    import torch
    if not H.is_cuda:
        raise ValueError("qpb.factor_box expects a CUDA (HIP) tensor; use factor_box_host for numpy")
    if H.dtype != torch.float64 or not H.is_contiguous():
        raise ValueError("inputs must be contiguous float64")
    n = H.shape[-1]
    if tuple(H.shape) != (n, n):
        raise ValueError("shape mismatch: H must be (n, n)")
    fac = torch.empty((factor_box_doubles(n),), dtype=torch.float64, device=H.device)
    status = torch.empty((1,), dtype=torch.int32, device=H.device)
    rc = _lib.qpb_factor_box(n, _ptr(H), _ptr(fac), _ptr(status), _stream_ptr(stream))
    _check(rc, "qpb_factor_box")
    return BoxFactor(fac, n, status)


def solve_box_factored(F: BoxFactor, f, lb=None, ub=None, *, max_iter: int = 0, feas_tol: float = 0.0,
                       out: Solution | None = None, stream=None) -> Solution:
    """``solve_box_shared`` without the per-QP set-up (qpb_solve_box_factored):
    ``F`` is ``factor_box(H)``, f (B, n) and lb / ub (B, n) or None are per QP.
    The contract is ``solve_box_shared``'s except that x and lam may differ from
    it by rounding and ``iters`` need not be the same."""
    import torch
    if not (f.is_cuda and F.fac.is_cuda):
        raise ValueError("qpb.solve_box_factored expects CUDA (HIP) tensors; use solve_box_factored_host for numpy")
    n = int(F.n)
    for t in (f, lb, ub):
        if t is not None and (t.dtype != torch.float64 or not t.is_contiguous()):
            raise ValueError("inputs must be contiguous float64")
        if t is not None and t.device != F.fac.device:
            raise ValueError("the inputs must live on the factor's CUDA device")
    if f.dim() != 2 or f.shape[1] != n or any(t is not None and t.shape != f.shape for t in (lb, ub)):
        raise ValueError(f"shape mismatch: the factor is for n={n}")
    if F.fac.dtype != torch.float64 or tuple(F.fac.shape) != (factor_box_doubles(n),) or not F.fac.is_contiguous():
        raise ValueError(f"the factor buffer is not one for n={n}")
    B, m = f.shape[0], 2 * n
    if out is None:
        out = _empty_solution(B, n, m, f.device)
    d = Desc(n, m, B, max_iter, 0, feas_tol)
    rc = _lib.qpb_solve_box_factored(ctypes.byref(d), _ptr(F.fac), _ptr(f), _ptr(lb), _ptr(ub), _ptr(out.x),
                                     _ptr(out.lam), _ptr(out.active), _ptr(out.status), _ptr(out.iters),
                                     _stream_ptr(stream))
    _check(rc, "qpb_solve_box_factored")
    return out


def factor_box_host(H) -> BoxFactor:
    """numpy in / numpy out (qpb_factor_box_host): ``factor_box`` with a host array."""
    import numpy as np
    H = np.ascontiguousarray(H, dtype=np.float64)
    n = H.shape[-1]
    if H.shape != (n, n):
        raise ValueError("shape mismatch: H must be (n, n)")
    fac = np.zeros(factor_box_doubles(n))
    st = np.zeros(1, dtype=np.int32)
    rc = _lib.qpb_factor_box_host(n, H.ctypes.data_as(ctypes.c_void_p), fac.ctypes.data_as(ctypes.c_void_p),
                                  st.ctypes.data_as(ctypes.c_void_p))
    _check(rc, "qpb_factor_box_host")
    return BoxFactor(fac, n, st)


def solve_box_factored_host(F: BoxFactor, f, lb=None, ub=None, *, max_iter: int = 0,
                            feas_tol: float = 0.0) -> Solution:
    """numpy in / numpy out (qpb_solve_box_factored_host): ``solve_box_factored`` with host arrays."""
    import numpy as np
    n = int(F.n)
    fac = np.ascontiguousarray(F.fac, dtype=np.float64)
    f = np.ascontiguousarray(f, dtype=np.float64)
    lb = None if lb is None else np.ascontiguousarray(lb, dtype=np.float64)
    ub = None if ub is None else np.ascontiguousarray(ub, dtype=np.float64)
    B = f.shape[0]
    if f.shape != (B, n) or any(t is not None and t.shape != (B, n) for t in (lb, ub)) or \
            fac.shape != (factor_box_doubles(n),):
        raise ValueError(f"shape mismatch: the factor is for n={n}")
    m = 2 * n
    x = np.zeros((B, n))
    lam = np.zeros((B, m))
    act = np.zeros((B, (m + 31) // 32), dtype=np.uint32)
    st = np.zeros(B, dtype=np.int32)
    it = np.zeros(B, dtype=np.int32)
    d = Desc(n, m, B, max_iter, 0, feas_tol)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None  # noqa: E731
    rc = _lib.qpb_solve_box_factored_host(ctypes.byref(d), p(fac), p(f), p(lb), p(ub), p(x), p(lam), p(act), p(st),
                                          p(it))
    _check(rc, "qpb_solve_box_factored_host")
    return Solution(x, lam, act, st, it)


def solve_box_shared_backward(H, sol: Solution, gx, *, need=BOX_NEED_ALL, stream=None):
    """``solve_box_backward`` with ONE H (n, n) (qpb_solve_box_shared_backward):
    given ``sol`` from ``solve_box_shared`` on (H, f, lb, ub) and the cotangent
    ``gx`` (B, n), returns ``(gH, gf, glb, gub)``: gf, glb and gub (B, n) are
    ``solve_box_backward``'s bit for bit, and gH is ONE (n, n) matrix, the sum
    over the batch of the per-QP dl/dH, computed on the matrix cores without a
    per-QP copy and without atomics (its bits depend on the inputs and on
    (n, B) only).  QPs whose status is not OK contribute exactly 0.  ``need``
    and ``sol.status`` as for ``solve_box_backward``.  n <= 32.
    """
    import torch
    if not (H.is_cuda and gx.is_cuda):
        raise ValueError("qpb.solve_box_shared_backward expects CUDA (HIP) tensors; "
                         "use solve_box_shared_backward_host for numpy")
    B, n = gx.shape
    for t in (H, gx):
        if t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError("inputs must be contiguous float64")
    if H.shape != (n, n):
        raise ValueError("shape mismatch: H must be (n, n)")
    need = _box_need_set(need)
    if not sol.x.is_cuda or sol.x.dtype != torch.float64 or not sol.x.is_contiguous() or sol.x.shape != (B, n):
        raise ValueError("sol.x must be a contiguous float64 CUDA tensor of shape (B, n)")
    if (sol.active is None or not sol.active.is_cuda or not sol.active.is_contiguous()
            or sol.active.shape != (B, (2 * n + 31) // 32) or sol.active.element_size() != 4):
        raise ValueError("sol.active must be a contiguous (B, ceil(2n/32)) CUDA tensor of 32-bit words")
    if sol.status is not None and (sol.status.dtype != torch.int32 or not sol.status.is_contiguous()
                                   or sol.status.shape != (B,)):
        raise ValueError("sol.status must be a contiguous int32 tensor of shape (B,) or None")
    dev = gx.device
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)  # noqa: E731
    gH = new(n, n) if "H" in need else None
    gf = new(B, n) if "f" in need else None
    glb = new(B, n) if "lb" in need else None
    gub = new(B, n) if "ub" in need else None
    d = Desc(n, 2 * n, B, 0, 0, 0.0)
    rc = _lib.qpb_solve_box_shared_backward(ctypes.byref(d), _ptr(H), _ptr(sol.x), _ptr(sol.active),
                                            _ptr(sol.status), _ptr(gx), _ptr(gH), _ptr(gf), _ptr(glb), _ptr(gub),
                                            _stream_ptr(stream))
    _check(rc, "qpb_solve_box_shared_backward")
    return gH, gf, glb, gub


def solve_box_shared_backward_host(H, sol: Solution, gx, *, need=BOX_NEED_ALL):
    """numpy in / numpy out (qpb_solve_box_shared_backward_host): ``solve_box_shared_backward`` with host arrays."""
    import numpy as np
    need = _box_need_set(need)
    H = np.ascontiguousarray(H, dtype=np.float64)
    gx = np.ascontiguousarray(gx, dtype=np.float64)
    x = np.ascontiguousarray(sol.x, dtype=np.float64)
    B, n = gx.shape
    act = np.ascontiguousarray(np.asarray(sol.active).astype(np.uint32))
    if H.shape != (n, n) or x.shape != (B, n) or act.shape != (B, (2 * n + 31) // 32):
        raise ValueError("shape mismatch")
    st = None if sol.status is None else np.ascontiguousarray(sol.status, dtype=np.int32)
    gH = np.zeros((n, n)) if "H" in need else None
    gf = np.zeros((B, n)) if "f" in need else None
    glb = np.zeros((B, n)) if "lb" in need else None
    gub = np.zeros((B, n)) if "ub" in need else None
    d = Desc(n, 2 * n, B, 0, 0, 0.0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None  # noqa: E731
    rc = _lib.qpb_solve_box_shared_backward_host(ctypes.byref(d), p(H), p(x), p(act), p(st), p(gx), p(gH), p(gf),
                                                 p(glb), p(gub))
    _check(rc, "qpb_solve_box_shared_backward_host")
    return gH, gf, glb, gub


def solve_box_backward_dual(H, sol: Solution, gx, glam, *, need=BOX_NEED_ALL, stream=None):
    """``solve_box_backward`` (H (B, n, n)) or ``solve_box_shared_backward`` (a
    2-D H (n, n): gH is ONE matrix, the sum over the batch) for a loss that also
    reads the multipliers (qpb_solve_box_backward_dual).  ``glam = dl/dlam`` is
    (B, 2n) in ``solve_box``'s lam layout, the upper bounds' entries first; on
    unit rows it is a prescribed dx on the fixed variables (qpb.h has the
    contract).  ``glam`` of a bound that is not active, of the lower bound of a
    variable whose both bits are set and of QPs whose status is not OK is
    ignored, whatever it holds.  ``glam=None`` is the call without it, bit for
    bit.  n <= 32."""
    import torch
    if not (H.is_cuda and gx.is_cuda):
        raise ValueError("qpb.solve_box_backward_dual expects CUDA (HIP) tensors; "
                         "use solve_box_backward_dual_host for numpy")
    if glam is None:
        return (solve_box_shared_backward if H.dim() == 2 else solve_box_backward)(H, sol, gx, need=need,
                                                                                  stream=stream)
    B, n = gx.shape
    for t in (H, gx, glam):
        if not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError("inputs must be contiguous float64 CUDA tensors")
    shared = SHARED_H if H.dim() == 2 else 0
    if tuple(H.shape) != ((n, n) if shared else (B, n, n)) or tuple(glam.shape) != (B, 2 * n):
        raise ValueError("shape mismatch: H must be (n, n) or (B, n, n) and glam (B, 2n)")
    need = _box_need_set(need)
    if not sol.x.is_cuda or sol.x.dtype != torch.float64 or not sol.x.is_contiguous() or sol.x.shape != (B, n):
        raise ValueError("sol.x must be a contiguous float64 CUDA tensor of shape (B, n)")
    if (sol.active is None or not sol.active.is_cuda or not sol.active.is_contiguous()
            or sol.active.shape != (B, (2 * n + 31) // 32) or sol.active.element_size() != 4):
        raise ValueError("sol.active must be a contiguous (B, ceil(2n/32)) CUDA tensor of 32-bit words")
    if sol.status is not None and (sol.status.dtype != torch.int32 or not sol.status.is_contiguous()
                                   or sol.status.shape != (B,)):
        raise ValueError("sol.status must be a contiguous int32 tensor of shape (B,) or None")
    dev = gx.device
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)  # noqa: E731
    gH = new(*H.shape) if "H" in need else None
    gf = new(B, n) if "f" in need else None
    glb = new(B, n) if "lb" in need else None
    gub = new(B, n) if "ub" in need else None
    d = Desc(n, 2 * n, B, 0, 0, 0.0)
    rc = _lib.qpb_solve_box_backward_dual(ctypes.byref(d), shared, _ptr(H), _ptr(sol.x), _ptr(sol.active),
                                          _ptr(sol.status), _ptr(gx), _ptr(glam), _ptr(gH), _ptr(gf), _ptr(glb),
                                          _ptr(gub), _stream_ptr(stream))
    _check(rc, "qpb_solve_box_backward_dual")
    return gH, gf, glb, gub


def solve_box_backward_dual_host(H, sol: Solution, gx, glam, *, need=BOX_NEED_ALL):
    """numpy in / numpy out (qpb_solve_box_backward_dual_host): ``solve_box_backward_dual`` with host arrays."""
    import numpy as np
    need = _box_need_set(need)
    H = np.ascontiguousarray(H, dtype=np.float64)
    gx = np.ascontiguousarray(gx, dtype=np.float64)
    x = np.ascontiguousarray(sol.x, dtype=np.float64)
    B, n = gx.shape
    act = np.ascontiguousarray(np.asarray(sol.active).astype(np.uint32))
    glam = None if glam is None else np.ascontiguousarray(glam, dtype=np.float64)
    shared = SHARED_H if H.ndim == 2 else 0
    if H.shape != ((n, n) if shared else (B, n, n)) or x.shape != (B, n) or act.shape != (B, (2 * n + 31) // 32) \
            or (glam is not None and glam.shape != (B, 2 * n)):
        raise ValueError("shape mismatch")
    st = None if sol.status is None else np.ascontiguousarray(sol.status, dtype=np.int32)
    gH = np.zeros(H.shape) if "H" in need else None
    gf = np.zeros((B, n)) if "f" in need else None
    glb = np.zeros((B, n)) if "lb" in need else None
    gub = np.zeros((B, n)) if "ub" in need else None
    d = Desc(n, 2 * n, B, 0, 0, 0.0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None  # noqa: E731
    rc = _lib.qpb_solve_box_backward_dual_host(ctypes.byref(d), shared, p(H), p(x), p(act), p(st), p(gx), p(glam),
                                               p(gH), p(gf), p(glb), p(gub))
    _check(rc, "qpb_solve_box_backward_dual_host")
    return gH, gf, glb, gub


def solve_box_tangent(H, sol: Solution, df, dlb=None, dub=None, *, stream=None):
    """The forward sensitivity of a box solve: the tangent ``(dx, dlam)`` of
    (x*, lam*) along a change ``df`` of f and ``dlb``, ``dub`` (B, n) of the
    bounds, at fixed active set; ``dlam`` is (B, 2n) in ``solve_box``'s lam
    layout.  ONE call of ``solve_box_backward_dual`` with ``gx = df``,
    ``glam[:, :n] = -dub``, ``glam[:, n:] = +dlb`` and ``need = ("f", "lb",
    "ub")``: ``dx = gf``, ``dlam = [-gub, +glb]``.  A fixed variable moves with
    its bound and a free one follows through H; ``dlam`` is 0 on a bound that
    is not active.  H (B, n, n), or (n, n) for one H.  With ``dlb`` and ``dub``
    None the bounds do not move and the call runs the box backward's kernels."""
    import contextlib

    import torch
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        glam = None
        if dlb is not None or dub is not None:
            z = torch.zeros_like(df)
            glam = torch.cat((z if dub is None else -dub, z if dlb is None else dlb), dim=1).contiguous()
        _, dx, glb, gub = solve_box_backward_dual(H, sol, df, glam, need=("f", "lb", "ub"), stream=stream)
        return dx, torch.cat((-gub, glb), dim=1)


# ---- T right-hand sides per QP in one launch -----------------------------------
MULTI_NEED_ALL = ("f", "b")
BOX_MULTI_NEED_ALL = ("f", "lb", "ub")


def _multi_need_set(need, names) -> set:
    need = set(need)
    if not need or not need <= set(names):
        raise ValueError(f"need must be a non-empty subset of {names}")
    return need


def _multi_dims(gx, n: int, B: int):
    """(T, shared bit) of right-hand sides (B, T, n), or (T, n) for one set that
    every QP reads."""
    if gx.ndim == 3 and tuple(gx.shape[::2]) == (B, n):
        T, sh = int(gx.shape[1]), 0
    elif gx.ndim == 2 and gx.shape[1] == n:
        T, sh = int(gx.shape[0]), SHARED_RHS
    else:
        raise ValueError(f"shape mismatch: gx must be (B, T, n) or (T, n) with B={B}, n={n}")
    if not 1 <= T <= MAX_RHS:
        raise ValueError(f"the number of right-hand sides T must be 1..{MAX_RHS} (got {T})")
    return T, sh


def _multi_sol_batch(sol: Solution) -> int:
    lead = sol.active if sol.active is not None else sol.status
    if lead is None:
        raise ValueError("sol.active or sol.status must give the batch size")
    return int(lead.shape[0])


def _multi_check_sol_cuda(sol: Solution, B: int, words: int, dev):
    import torch
    if words and (sol.active is None or not sol.active.is_cuda or not sol.active.is_contiguous()
                  or tuple(sol.active.shape) != (B, words) or sol.active.element_size() != 4
                  or sol.active.device != dev):
        raise ValueError("sol.active must be a contiguous (B, ceil(m/32)) CUDA tensor of 32-bit words")
    if sol.status is not None and (not sol.status.is_cuda or sol.status.dtype != torch.int32
                                   or not sol.status.is_contiguous() or tuple(sol.status.shape) != (B,)):
        raise ValueError("sol.status must be a contiguous int32 tensor of shape (B,) or None")


def solve_factored_backward_multi(F: BackwardFactor, sol: Solution, gx, glam=None, *, need=MULTI_NEED_ALL,
                                  stream=None):
    """T right-hand sides per QP in ONE launch (qpb_solve_factored_backward_multi):
    ``solve_factored_backward_dual(F, sol, gx[:, t], glam[:, t], need=("f", "b"))``
    for every direction t, bit for bit, with the factored load and the
    orthogonalisation done once per QP.  ``gx`` is (B, T, n) and ``glam``
    (B, T, m), or (T, n) and (T, m) for ONE set that every QP reads (B is taken
    from ``sol.active`` / ``sol.status``).  Returns (gf (B, T, n), gb (B, T, m));
    an entry is None where ``need`` leaves it out, and gb with m == 0.  Only
    ``sol.active`` and ``sol.status`` are read.  ``glam=None`` (or m = 0) is
    ``solve_factored_backward`` per direction.  n <= 32, m <= 64, T <= 256."""
    import torch
    if not (gx.is_cuda and F.fac.is_cuda):
        raise ValueError("qpb.solve_factored_backward_multi expects CUDA (HIP) tensors; "
                         "use solve_factored_backward_multi_host for numpy")
    n, m = int(F.n), int(F.m)
    need = _multi_need_set(need, MULTI_NEED_ALL)
    if gx.dtype != torch.float64 or not gx.is_contiguous():
        raise ValueError("inputs must be contiguous float64")
    B = _multi_sol_batch(sol)
    T, shared = _multi_dims(gx, n, B)
    if F.fac.dtype != torch.float64 or tuple(F.fac.shape) != (factor_backward_doubles(n, m),) \
            or not F.fac.is_contiguous():
        raise ValueError(f"the backward factor buffer is not one for n={n}, m={m}")
    if F.fac.device != gx.device:
        raise ValueError("the inputs must live on the factor's CUDA device")
    _multi_check_sol_cuda(sol, B, (m + 31) // 32, gx.device)
    if glam is not None and (not glam.is_cuda or glam.dtype != torch.float64 or not glam.is_contiguous()
                             or glam.device != gx.device or tuple(glam.shape) != tuple(gx.shape[:-1]) + (m,)):
        raise ValueError("glam must be a contiguous float64 CUDA tensor of gx's shape with m in place of n, or None")
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=gx.device)  # noqa: E731
    gf = new(B, T, n) if "f" in need else None
    gb = new(B, T, m) if m and "b" in need else None
    if gf is None and gb is None:
        return None, None  # m == 0 and only b wanted
    d = Desc(n, m, B, 0, 0, 0.0)
    rc = _lib.qpb_solve_factored_backward_multi(ctypes.byref(d), _ptr(F.fac), _ptr(sol.active) if m else None,
                                                _ptr(sol.status), T, shared, _ptr(gx),
                                                _ptr(glam) if m and glam is not None else None, _ptr(gf), _ptr(gb),
                                                _stream_ptr(stream))
    _check(rc, "qpb_solve_factored_backward_multi")
    return gf, gb


def solve_factored_tangents(F: BackwardFactor, sol: Solution, df, db=None, *, stream=None):
    """``solve_factored_tangent`` for T directions in ONE launch: the tangents
    ``(dx, dlam)`` of (x*, lam*) along ``df`` (B, T, n) and ``db`` (B, T, m) --
    or (T, n) and (T, m) for directions that do not depend on the QP, the
    columns of an affine law -- at fixed active set: ``gx = df``,
    ``glam = -db``, ``dlam = -gb``.  Returns dx (B, T, n) and dlam (B, T, m)
    (None at m = 0), each direction bit for bit ``solve_factored_tangent``'s."""
    import contextlib

    import torch
    m = int(F.m)
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        glam = None if db is None or not m else -db
        dx, gb = solve_factored_backward_multi(F, sol, df, glam, need=("f", "b"), stream=stream)
        return dx, (None if gb is None else -gb)


def solve_factored_backward_multi_host(F: BackwardFactor, sol: Solution, gx, glam=None, *, need=MULTI_NEED_ALL):
    """numpy in / numpy out (qpb_solve_factored_backward_multi_host): ``solve_factored_backward_multi`` with host
    arrays."""
    import numpy as np
    need = _multi_need_set(need, MULTI_NEED_ALL)
    n, m = int(F.n), int(F.m)
    fac = np.ascontiguousarray(F.fac, dtype=np.float64)
    gx = np.ascontiguousarray(gx, dtype=np.float64)
    B = _multi_sol_batch(sol)
    T, shared = _multi_dims(gx, n, B)
    act = None
    if m:
        act = np.ascontiguousarray(np.asarray(sol.active).astype(np.uint32))
    if fac.shape != (factor_backward_doubles(n, m),) or (m and act.shape != (B, (m + 31) // 32)):
        raise ValueError(f"shape mismatch: the factor is for n={n}, m={m}")
    glam = None if glam is None or not m else np.ascontiguousarray(glam, dtype=np.float64)
    if glam is not None and glam.shape != gx.shape[:-1] + (m,):
        raise ValueError(f"shape mismatch: the factor is for n={n}, m={m}")
    st = None if sol.status is None else np.ascontiguousarray(sol.status, dtype=np.int32)
    if st is not None and st.shape != (B,):
        raise ValueError("shape mismatch: sol.status must be (B,)")
    gf = np.zeros((B, T, n)) if "f" in need else None
    gb = np.zeros((B, T, m)) if m and "b" in need else None
    if gf is None and gb is None:
        return None, None
    d = Desc(n, m, B, 0, 0, 0.0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None  # noqa: E731
    rc = _lib.qpb_solve_factored_backward_multi_host(ctypes.byref(d), p(fac), p(act), p(st), T, shared, p(gx),
                                                     p(glam), p(gf), p(gb))
    _check(rc, "qpb_solve_factored_backward_multi_host")
    return gf, gb


def solve_box_backward_multi(H, sol: Solution, gx, glam=None, *, need=BOX_MULTI_NEED_ALL, stream=None):
    """T right-hand sides per QP in ONE launch (qpb_solve_box_backward_multi):
    ``solve_box_backward_dual(H, sol, gx[:, t], glam[:, t], need=("f", "lb",
    "ub"))`` for every direction t, bit for bit, with H loaded and the masked
    Cholesky done once per QP.  H is (B, n, n), or (n, n) for one H; ``gx`` is
    (B, T, n) and ``glam`` (B, T, 2n), or (T, n) and (T, 2n) for ONE set that
    every QP reads (B is taken from ``sol.active``).  Returns (gf, glb, gub),
    each (B, T, n), None where ``need`` leaves it out.  Only ``sol.active`` and
    ``sol.status`` are read.  ``glam=None`` is ``solve_box_backward`` per
    direction.  n <= 32, T <= 256."""
    import torch
    if not (H.is_cuda and gx.is_cuda):
        raise ValueError("qpb.solve_box_backward_multi expects CUDA (HIP) tensors; "
                         "use solve_box_backward_multi_host for numpy")
    for t in (H, gx) + (() if glam is None else (glam,)):
        if not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError("inputs must be contiguous float64 CUDA tensors")
    n = int(H.shape[-1])
    B = _multi_sol_batch(sol)
    T, shared = _multi_dims(gx, n, B)
    if H.dim() == 2:
        shared |= SHARED_H
    if tuple(H.shape) != ((n, n) if H.dim() == 2 else (B, n, n)) \
            or (glam is not None and tuple(glam.shape) != tuple(gx.shape[:-1]) + (2 * n,)):
        raise ValueError("shape mismatch: H must be (n, n) or (B, n, n) and glam gx's shape with 2n in place of n")
    need = _multi_need_set(need, BOX_MULTI_NEED_ALL)
    _multi_check_sol_cuda(sol, B, (2 * n + 31) // 32, gx.device)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=gx.device)  # noqa: E731
    gf = new(B, T, n) if "f" in need else None
    glb = new(B, T, n) if "lb" in need else None
    gub = new(B, T, n) if "ub" in need else None
    d = Desc(n, 2 * n, B, 0, 0, 0.0)
    rc = _lib.qpb_solve_box_backward_multi(ctypes.byref(d), shared, _ptr(H), _ptr(sol.active), _ptr(sol.status), T,
                                           _ptr(gx), _ptr(glam), _ptr(gf), _ptr(glb), _ptr(gub), _stream_ptr(stream))
    _check(rc, "qpb_solve_box_backward_multi")
    return gf, glb, gub


def solve_box_tangents(H, sol: Solution, df, dlb=None, dub=None, *, stream=None):
    """``solve_box_tangent`` for T directions in ONE launch: the tangents
    ``(dx, dlam)`` of (x*, lam*) along ``df``, ``dlb`` and ``dub``, each
    (B, T, n) or, for directions that do not depend on the QP, (T, n); ``dlam``
    is (B, T, 2n) in ``solve_box``'s lam layout.  ``gx = df``,
    ``glam[..., :n] = -dub``, ``glam[..., n:] = +dlb``, ``dx = gf``,
    ``dlam = [-gub, +glb]``: each direction bit for bit ``solve_box_tangent``'s."""
    import contextlib

    import torch
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        glam = None
        if dlb is not None or dub is not None:
            z = torch.zeros_like(df)
            glam = torch.cat((z if dub is None else -dub, z if dlb is None else dlb), dim=-1).contiguous()
        dx, glb, gub = solve_box_backward_multi(H, sol, df, glam, need=("f", "lb", "ub"), stream=stream)
        return dx, torch.cat((-gub, glb), dim=-1)


def solve_box_backward_multi_host(H, sol: Solution, gx, glam=None, *, need=BOX_MULTI_NEED_ALL):
    """numpy in / numpy out (qpb_solve_box_backward_multi_host): ``solve_box_backward_multi`` with host arrays."""
    import numpy as np
    need = _multi_need_set(need, BOX_MULTI_NEED_ALL)
    H = np.ascontiguousarray(H, dtype=np.float64)
    gx = np.ascontiguousarray(gx, dtype=np.float64)
    n = H.shape[-1]
    B = _multi_sol_batch(sol)
    T, shared = _multi_dims(gx, n, B)
    if H.ndim == 2:
        shared |= SHARED_H
    act = np.ascontiguousarray(np.asarray(sol.active).astype(np.uint32))
    glam = None if glam is None else np.ascontiguousarray(glam, dtype=np.float64)
    if H.shape != ((n, n) if H.ndim == 2 else (B, n, n)) or act.shape != (B, (2 * n + 31) // 32) \
            or (glam is not None and glam.shape != gx.shape[:-1] + (2 * n,)):
        raise ValueError("shape mismatch")
    st = None if sol.status is None else np.ascontiguousarray(sol.status, dtype=np.int32)
    if st is not None and st.shape != (B,):
        raise ValueError("shape mismatch: sol.status must be (B,)")
    gf = np.zeros((B, T, n)) if "f" in need else None
    glb = np.zeros((B, T, n)) if "lb" in need else None
    gub = np.zeros((B, T, n)) if "ub" in need else None
    d = Desc(n, 2 * n, B, 0, 0, 0.0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None  # noqa: E731
    rc = _lib.qpb_solve_box_backward_multi_host(ctypes.byref(d), shared, p(H), p(act), p(st), T, p(gx), p(glam),
                                                p(gf), p(glb), p(gub))
    _check(rc, "qpb_solve_box_backward_multi_host")
    return gf, glb, gub


def active_mask_to_bool(active, m: int):
    """(B, words) uint32/int32 bit words -> (B, m) bool (numpy)."""
    import numpy as np
    a = np.asarray(active).astype(np.uint32)
    bits = ((a[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool)
    return bits.reshape(a.shape[0], -1)[:, :m]


def _require_f64_cuda(name: str, t, shape: tuple):
    """A contiguous float64 CUDA tensor of exactly `shape`: the C-ABI reads
    the pointer as device memory of that layout, so a CPU tensor, another
    dtype or a strided view must be refused here, not dereferenced there."""
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
            and tuple(t.shape) == tuple(shape)):
        got = (tuple(t.shape), str(t.dtype), str(t.device), t.is_contiguous()) if isinstance(t, torch.Tensor) \
            else type(t).__name__
        raise ValueError(f"{name}: expected a contiguous float64 CUDA tensor of shape {tuple(shape)}, got {got}")


def ref_solve(mode: int, P, q, x0=None, *, iterations: int, box=(-1e12, 1e12), stream=None):
    """Reference-semantics batched solvers (qp_solvers.c replicas) on CUDA tensors:
    P (B, n, n), q (B, n), x0 (B, n) or None: zeros for GD and Newton, unused
    by ADMM (qp_solvers.c:256 ignores its x0)."""
    import torch
    if not (isinstance(q, torch.Tensor) and q.dim() == 2):
        raise ValueError("qpb.ref_solve: q must be a (B, n) tensor")
    B, n = q.shape
    _require_f64_cuda("qpb.ref_solve: q", q, (B, n))
    _require_f64_cuda("qpb.ref_solve: P", P, (B, n, n))
    if x0 is not None:
        _require_f64_cuda("qpb.ref_solve: x0", x0, (B, n))
        if x0.device != q.device or P.device != q.device:
            raise ValueError("qpb.ref_solve: P, q and x0 must be on one device")
    elif P.device != q.device:
        raise ValueError("qpb.ref_solve: P and q must be on one device")
    elif mode != REF_ADMM:
        # GD and Newton start from x0 (qpb_ref_solve requires it); ADMM ignores
        # it, as the reference does (qp_solvers.c:256)
        x0 = torch.zeros_like(q)
    x = torch.empty((B, n), dtype=torch.float64, device=q.device)
    it = torch.empty((B,), dtype=torch.int32, device=q.device)
    d = RefDesc(n, mode, B, iterations, 0, float(box[0]), float(box[1]))
    rc = _lib.qpb_ref_solve(ctypes.byref(d), _ptr(P), _ptr(q), _ptr(x0) if x0 is not None else None,
                            _ptr(x), _ptr(it), _stream_ptr(stream))
    _check(rc, "qpb_ref_solve")
    return x, it


_lib.qpb_release_stream_workspace.argtypes = [_vp]
_lib.qpb_release_stream_workspace.restype = ctypes.c_int
_lib.qpb_release_workspaces.argtypes = []
_lib.qpb_release_workspaces.restype = ctypes.c_int


def release_stream_workspace(stream=None) -> None:
    """qpb_release_stream_workspace: free the scratch buffer cached for
    `stream` (a torch.cuda.Stream or ExternalStream; None = the current
    stream).  The n <= 128 kernels and the reference replicas above n = 64
    cache one buffer per (device, stream) and free it stream-ordered on that
    stream, so call this before destroying a stream passed as ``stream=``."""
    _check(_lib.qpb_release_stream_workspace(_stream_ptr(stream)), "qpb_release_stream_workspace")


def release_workspaces() -> None:
    """qpb_release_workspaces: synchronise every cached stream and free all the scratch buffers."""
    _check(_lib.qpb_release_workspaces(), "qpb_release_workspaces")


def matrix_invert(P, stream=None):
    """Batched reference matrix_invert (matrix_ops.c:551-630) of (B, n, n) CUDA tensors."""
    import torch
    if not (P.is_cuda and P.dtype == torch.float64 and P.is_contiguous() and P.dim() == 3
            and P.shape[1] == P.shape[2]):
        raise ValueError("qpb.matrix_invert expects a contiguous float64 CUDA tensor of shape (B, n, n)")
    B, n, _ = P.shape
    out = torch.empty_like(P)
    _check(_lib.qpb_matrix_invert(n, B, _ptr(P), _ptr(out), _stream_ptr(stream)), "qpb_matrix_invert")
    return out


def qf_eval(P, q, r: float, x, stream=None):
    """Batched quadratic_form_eval (qp.c:9-27): 1/2 x'Px + q'x + r per QP;
    P (B, n, n), q (B, n), x (B, n) float64 CUDA tensors."""
    import torch
    if not (isinstance(q, torch.Tensor) and q.dim() == 2):
        raise ValueError("qpb.qf_eval: q must be a (B, n) tensor")
    B, n = q.shape
    _require_f64_cuda("qpb.qf_eval: q", q, (B, n))
    _require_f64_cuda("qpb.qf_eval: P", P, (B, n, n))
    _require_f64_cuda("qpb.qf_eval: x", x, (B, n))
    if not (P.device == q.device == x.device):
        raise ValueError("qpb.qf_eval: P, q and x must be on one device")
    out = torch.empty((B,), dtype=torch.float64, device=q.device)
    rc = _lib.qpb_qf_eval(n, B, _ptr(P), _ptr(q), float(r), _ptr(x), _ptr(out), _stream_ptr(stream))
    _check(rc, "qpb_qf_eval")
    return out


_lib.qpb_solve_sections.argtypes = [ctypes.POINTER(Desc)] + [_vp] * 10 + [ctypes.c_int64, _vp]
_lib.qpb_solve_sections.restype = ctypes.c_int
SECTION_NAMES = ["load", "cholesky", "substitution", "init", "select", "exchange", "back_solve", "step",
                 "add", "drop", "loop_exit", "output"]
N_SECTIONS = 20  # kSections (csrc/qpb_common.h): every stamped kernel adds all of them into the buffer
SECTION_SLOTS = 256  # kSectionSlots: rows of the device buffer (one per blockIdx mod 256)
WAVE_SECTION_NAMES = ["load", "sweep", "init", "select", "exchange", "back_solve", "step", "add", "drop",
                      "loop_exit", "x", "stores"]


def solve_sections(H, f, A, b, sections, *, max_iter: int = 0, out: Solution | None = None, stream=None):
    """Diagnostic builds of the n=16 (16<m<=32), 16<n<=32 (m<=64) and Gram
    (32<n<=128 or m>64, up to m=256; one launch, so a batch within the route's
    step) kernels: accumulate per-section wave ticks (100 MHz) into the int64
    CUDA tensor ``sections`` (N_SECTIONS = 20 int64 entries; the first 12 are
    named by SECTION_NAMES / WAVE_SECTION_NAMES for the first two builds; the
    Gram build stamps the first workgroup wave's ticks into 19 of them)."""
    import torch
    if not (sections.is_cuda and sections.dtype == torch.int64 and sections.is_contiguous()
            and sections.numel() >= N_SECTIONS):
        raise ValueError(f"sections must be a contiguous int64 CUDA tensor of >= {N_SECTIONS} entries")
    B, n = f.shape
    m = A.shape[1]
    if out is None:
        out = solve(H, f, A, b, max_iter=max_iter, stream=stream)
    d = Desc(n, m, B, max_iter, 0, 0.0)
    rows = torch.zeros((SECTION_SLOTS, N_SECTIONS), dtype=torch.int64, device=sections.device)
    rc = _lib.qpb_solve_sections(ctypes.byref(d), _ptr(H), _ptr(f), _ptr(A), _ptr(b), _ptr(out.x), _ptr(out.lam),
                                 _ptr(out.active), _ptr(out.status), _ptr(out.iters), _ptr(rows), rows.numel(),
                                 _stream_ptr(stream))
    _check(rc, "qpb_solve_sections")
    sections[:N_SECTIONS] += rows.sum(0)
    return out


# ------------------------------------------------------------------ generators
class RefGenDesc(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("seed", ctypes.c_uint32), ("batch", ctypes.c_int64),
                ("first", ctypes.c_uint64), ("p_min", ctypes.c_double), ("p_max", ctypes.c_double),
                ("q_min", ctypes.c_double), ("q_max", ctypes.c_double),
                ("x_min", ctypes.c_double), ("x_max", ctypes.c_double)]


class GenDesc(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("m", ctypes.c_int32), ("batch", ctypes.c_int64),
                ("first", ctypes.c_uint64), ("seed", ctypes.c_uint64), ("family", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("shift", ctypes.c_double), ("box", ctypes.c_double)]


FAMILY_BOX, FAMILY_DENSE = 0, 1
FAMILIES = {"box": FAMILY_BOX, "dense": FAMILY_DENSE}
_lib.qpb_ref_generate.argtypes = [ctypes.POINTER(RefGenDesc), _vp, _vp, _vp, _vp]
_lib.qpb_ref_generate.restype = ctypes.c_int
_lib.qpb_generate.argtypes = [ctypes.POINTER(GenDesc), _vp, _vp, _vp, _vp, _vp]
_lib.qpb_generate.restype = ctypes.c_int


def ref_generate(n: int, batch: int, seed: int, *, first: int = 0, p_range=(-1e3, 1e3), q_range=(-1e3, 1e3),
                 x_range=(-1e3, 1e3), device=None, stream=None):
    """The reference generator (srand(seed); main.c:37-39 order) on the GPU,
    QPs [first, first + batch): (P (B,n,n), q (B,n), x0 (B,n)) CUDA tensors."""
    import torch
    dev = device or torch.device("cuda", torch.cuda.current_device())
    P = torch.empty((batch, n, n), dtype=torch.float64, device=dev)
    q = torch.empty((batch, n), dtype=torch.float64, device=dev)
    x0 = torch.empty((batch, n), dtype=torch.float64, device=dev)
    d = RefGenDesc(n, seed & 0xFFFFFFFF, batch, first, *p_range, *q_range, *x_range)
    _check(_lib.qpb_ref_generate(ctypes.byref(d), _ptr(P), _ptr(q), _ptr(x0), _stream_ptr(stream)),
           "qpb_ref_generate")
    return P, q, x0


def generate(n: int, batch: int, seed: int, *, family: str = "box", m: int | None = None, first: int = 0,
             shift: float = 1.0, box: float = 10.0, device=None, stream=None):
    """Benchmark-family QPs from the counter-based generator (qpb_generate):
    (H, f, A, b) CUDA tensors; QP first + k is the same for any launch."""
    import torch
    dev = device or torch.device("cuda", torch.cuda.current_device())
    m = 2 * n if m is None else m
    H = torch.empty((batch, n, n), dtype=torch.float64, device=dev)
    f = torch.empty((batch, n), dtype=torch.float64, device=dev)
    A = torch.empty((batch, m, n), dtype=torch.float64, device=dev)
    b = torch.empty((batch, m), dtype=torch.float64, device=dev)
    d = GenDesc(n, m, batch, first, seed, FAMILIES[family], 0, shift, box)
    _check(_lib.qpb_generate(ctypes.byref(d), _ptr(H), _ptr(f), _ptr(A), _ptr(b), _stream_ptr(stream)),
           "qpb_generate")
    return H, f, A, b


# ------------------------------------------------------------------ wire format
_lib.qpb_wire_write.argtypes = [ctypes.c_char_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64] + [_vp] * 4
_lib.qpb_wire_write.restype = ctypes.c_int
_lib.qpb_wire_read_header.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int32),
                                      ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)]
_lib.qpb_wire_read_header.restype = ctypes.c_int
_lib.qpb_wire_read.argtypes = [ctypes.c_char_p] + [_vp] * 4
_lib.qpb_wire_read.restype = ctypes.c_int


def wire_write(path: str, H, f, A=None, b=None) -> None:
    """numpy (B,n,n), (B,n)[, (B,m,n), (B,m)] -> wire file (qpb_wire_write);
    a single unconstrained QP is written in the reference's own format."""
    import numpy as np
    H = np.ascontiguousarray(H, dtype=np.float64)
    f = np.ascontiguousarray(f, dtype=np.float64)
    B, n = f.shape
    m = 0 if A is None else A.shape[1]
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None  # noqa: E731
    if m:
        A = np.ascontiguousarray(A, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
    _check(_lib.qpb_wire_write(os.fsencode(path), n, m, B, p(H), p(f), p(A), p(b)), "qpb_wire_write")


def wire_read(path: str):
    """wire file -> numpy (H, f, A, b) (A, b have m = 0 columns for an unconstrained file)."""
    import numpy as np
    n, m, B = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
    _check(_lib.qpb_wire_read_header(os.fsencode(path), ctypes.byref(n), ctypes.byref(m), ctypes.byref(B)),
           "qpb_wire_read_header")
    n, m, B = n.value, m.value, B.value
    H, f = np.empty((B, n, n)), np.empty((B, n))
    A, b = np.empty((B, m, n)), np.empty((B, m))
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a.size else None  # noqa: E731
    _check(_lib.qpb_wire_read(os.fsencode(path), p(H), p(f), p(A), p(b)), "qpb_wire_read")
    return H, f, A, b
