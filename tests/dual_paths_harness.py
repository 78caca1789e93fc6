"""TEST INFRASTRUCTURE ONLY: C-ABI callers of qpb_solve_backward_dual,
qpb_solve_factored_backward_dual and qpb_solve_box_backward_dual for
tests/test_gpu_factored_backward_dual.py, tests/test_gpu_box_backward_dual.py
and tests/test_gpu_dual_paths_autograd.py, in tests/bwd_harness.py's manner.

Every call writes into buffers of its own, filled with 0xA5 and fenced by guard
words: every element of every non-NULL output must have been written and
nothing outside.  Inputs are numpy arrays; st None is status NULL and gl None
is glam NULL.
"""
import ctypes
import math

import numpy as np

from box_bwd_oracle import NAMES as BOX_NAMES
from bwd_harness import FILL8, GUARD, NAMES, dev


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _outputs(torch, shapes, need):
    bufs, views = {}, {}
    for k, shape in shapes.items():
        if k in need and math.prod(shape) > 0:
            t = torch.empty(math.prod(shape) + 2 * GUARD, dtype=torch.float64, device="cuda")
            t.view(torch.uint8).fill_(0xA5)
            bufs[k], views[k] = t, t[GUARD:GUARD + math.prod(shape)].view(shape)
    return bufs, views


def _collect(bufs, views):
    out = {}
    for k, t in bufs.items():
        raw = t.cpu().numpy().view(np.int64)
        assert (raw[:GUARD] == FILL8).all() and (raw[-GUARD:] == FILL8).all(), (k, "guard words written")
        assert not (raw[GUARD:-GUARD] == FILL8).any(), (k, "elements never written")
        out[k] = views[k].cpu().numpy()
    return out


def dual(qpb, shared, H, A, x, lam, act, st, g, gl, need=NAMES, stream=None):
    """qpb_solve_backward_dual: H is (n, n) with SHARED_H in `shared`, else
    (B, n, n), and A likewise.  Returns a dict of the numpy outputs in `need`."""
    import torch
    Bq, n = g.shape
    m = A.shape[-2]
    s = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(s):
        ins = [dev(H), dev(A) if m else None, dev(x), dev(lam) if m else None, dev(act) if m else None,
               dev(st) if st is not None else None, dev(g), dev(gl) if gl is not None and m else None]
        bufs, views = _outputs(torch, {"H": H.shape, "f": (Bq, n), "A": A.shape, "b": (Bq, m)}, need)
    d = qpb.Desc(n, m, Bq, 0, 0, 0.0)
    rc = qpb.lib().qpb_solve_backward_dual(ctypes.byref(d), shared, *[_ptr(t) for t in ins],
                                           *[_ptr(views.get(k)) for k in NAMES], ctypes.c_void_p(s.cuda_stream))
    assert rc == 0, qpb.lib().qpb_last_error()
    s.synchronize()
    return _collect(bufs, views)


def factored_dual(qpb, F, x, lam, act, st, g, gl, need=NAMES, stream=None):
    """qpb_solve_factored_backward_dual on a factored_bwd_cases.Factor: gH (n, n),
    gf (B, n), gA (m, n), gb (B, m); at m == 0 without A and b."""
    import torch
    Bq, n = g.shape
    m = F.m
    assert n == F.n
    s = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(s):
        ins = [dev(x), dev(lam) if m else None, dev(act) if m else None, dev(st) if st is not None else None, dev(g),
               dev(gl) if gl is not None and m else None]
        bufs, views = _outputs(torch, {"H": (n, n), "f": (Bq, n), "A": (m, n), "b": (Bq, m)}, need)
    d = qpb.Desc(n, m, Bq, 0, 0, 0.0)
    rc = qpb.lib().qpb_solve_factored_backward_dual(ctypes.byref(d), _ptr(F.fac), *[_ptr(t) for t in ins],
                                                    *[_ptr(views.get(k)) for k in NAMES],
                                                    ctypes.c_void_p(s.cuda_stream))
    assert rc == 0, qpb.lib().qpb_last_error()
    s.synchronize()
    return _collect(bufs, views)


def box_dual(qpb, shared, H, x, act, st, g, gl, need=BOX_NAMES, stream=None):
    """qpb_solve_box_backward_dual: H is (n, n) with `shared` = SHARED_H, else
    (B, n, n); gl (B, 2n).  Returns a dict over `need`: gH in H's shape, gf,
    glb, gub (B, n)."""
    import torch
    Bq, n = g.shape
    assert H.shape == ((n, n) if shared else (Bq, n, n))
    s = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(s):
        ins = [dev(H), dev(x), dev(act), dev(st) if st is not None else None, dev(g),
               dev(gl) if gl is not None else None]
        bufs, views = _outputs(torch, {"H": H.shape, "f": (Bq, n), "lb": (Bq, n), "ub": (Bq, n)}, need)
    d = qpb.Desc(n, 2 * n, Bq, 0, 0, 0.0)
    rc = qpb.lib().qpb_solve_box_backward_dual(ctypes.byref(d), shared, *[_ptr(t) for t in ins],
                                               *[_ptr(views.get(k)) for k in BOX_NAMES],
                                               ctypes.c_void_p(s.cuda_stream))
    assert rc == 0, qpb.lib().qpb_last_error()
    s.synchronize()
    return _collect(bufs, views)


def bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def same(got, ref, where):
    assert got.keys() == ref.keys(), (where, sorted(got), sorted(ref))
    for k in got:
        assert bits(got[k], ref[k]), (where, k, "differs bit for bit", float(np.nanmax(np.abs(got[k] - ref[k]))))
