"""TEST INFRASTRUCTURE ONLY: C-ABI callers of qpb_solve_factored_backward_multi
and qpb_solve_box_backward_multi for tests/test_gpu_factored_backward_multi.py
and tests/test_gpu_box_backward_multi.py, in tests/dual_paths_harness.py's
manner, and the single-direction references stacked over the directions.

Every call writes into buffers of its own, filled with 0xA5 and fenced by guard
words: every element of every non-NULL output must have been written and
nothing outside.  Inputs are numpy arrays; gx is (B, T, n), or (T, n) for
QPB_SHARED_RHS (one set of right-hand sides for the batch), and gl likewise or
None (glam NULL); st None is status NULL.
"""
import ctypes

import numpy as np

import dual_paths_harness as DP
from bwd_harness import dev

SHARED_H, SHARED_RHS = 1, 4
F_NAMES = ("f", "b")
BOX_NAMES = ("f", "lb", "ub")

_ptr = DP._ptr
bits, same = DP.bits, DP.same


def _dims(g, Bq):
    if g.ndim == 2:
        return g.shape[0], SHARED_RHS
    assert g.shape[0] == Bq
    return g.shape[1], 0


def factored_multi(qpb, F, act, st, g, gl, Bq, need=F_NAMES, stream=None):
    """qpb_solve_factored_backward_multi on a factored_bwd_cases.Factor: a dict
    over `need` of gf (B, T, n) and gb (B, T, m); at m == 0 without b."""
    import torch
    n, m = F.n, F.m
    assert g.shape[-1] == n and (gl is None or gl.shape == g.shape[:-1] + (m,))
    T, shared = _dims(g, Bq)
    s = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(s):
        ins = [dev(act) if m else None, dev(st) if st is not None else None]
        rhs = [dev(g), dev(gl) if gl is not None and m else None]
        bufs, views = DP._outputs(torch, {"f": (Bq, T, n), "b": (Bq, T, m)}, need)
    d = qpb.Desc(n, m, Bq, 0, 0, 0.0)
    rc = qpb.lib().qpb_solve_factored_backward_multi(ctypes.byref(d), _ptr(F.fac), *[_ptr(t) for t in ins], T, shared,
                                                     *[_ptr(t) for t in rhs], *[_ptr(views.get(k)) for k in F_NAMES],
                                                     ctypes.c_void_p(s.cuda_stream))
    assert rc == 0, qpb.lib().qpb_last_error()
    s.synchronize()
    return DP._collect(bufs, views)


def box_multi(qpb, shared_h, H, act, st, g, gl, Bq, need=BOX_NAMES, stream=None):
    """qpb_solve_box_backward_multi: H is (n, n) with `shared_h` = SHARED_H, else
    (B, n, n).  Returns a dict over `need` of gf, glb, gub (B, T, n)."""
    import torch
    n = g.shape[-1]
    assert H.shape == ((n, n) if shared_h else (Bq, n, n)) and (gl is None or gl.shape == g.shape[:-1] + (2 * n,))
    T, shared = _dims(g, Bq)
    s = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(s):
        ins = [dev(H), dev(act), dev(st) if st is not None else None]
        rhs = [dev(g), dev(gl) if gl is not None else None]
        bufs, views = DP._outputs(torch, {k: (Bq, T, n) for k in BOX_NAMES}, need)
    d = qpb.Desc(n, 2 * n, Bq, 0, 0, 0.0)
    rc = qpb.lib().qpb_solve_box_backward_multi(ctypes.byref(d), shared | shared_h, *[_ptr(t) for t in ins], T,
                                                *[_ptr(t) for t in rhs], *[_ptr(views.get(k)) for k in BOX_NAMES],
                                                ctypes.c_void_p(s.cuda_stream))
    assert rc == 0, qpb.lib().qpb_last_error()
    s.synchronize()
    return DP._collect(bufs, views)


def factored_single(qpb, F, x, lam, act, st, g, gl):
    """The existing single-direction call per direction, only the per-QP outputs
    asked for, stacked: a dict of gf (B, T, n) and gb (B, T, m) (no b at m == 0)."""
    T = g.shape[1]
    outs = [DP.factored_dual(qpb, F, x, lam, act, st, np.ascontiguousarray(g[:, t]),
                             None if gl is None else np.ascontiguousarray(gl[:, t]), need=F_NAMES) for t in range(T)]
    return {k: np.stack([o[k] for o in outs], axis=1) for k in outs[0]}


def box_single(qpb, shared_h, H, x, act, st, g, gl):
    """qpb_solve_box_backward_dual per direction, stacked: gf, glb, gub (B, T, n)."""
    T = g.shape[1]
    outs = [DP.box_dual(qpb, shared_h, H, x, act, st, np.ascontiguousarray(g[:, t]),
                        None if gl is None else np.ascontiguousarray(gl[:, t]), need=BOX_NAMES) for t in range(T)]
    return {k: np.stack([o[k] for o in outs], axis=1) for k in outs[0]}


def take(ref, T):
    """The first T directions of a stacked reference."""
    return {k: np.ascontiguousarray(v[:, :T]) for k, v in ref.items()}
