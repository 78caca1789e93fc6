"""TEST INFRASTRUCTURE ONLY: what the GPU tests of qpb_solve_box_shared and
qpb_solve_box_shared_backward share (tests/test_gpu_box_shared*.py), in
tests/box_bwd_harness.py's manner.

`solve` and `backward` call the C-ABI into buffers of their own, filled with
0xA5 and fenced by guard words, and check that every element was written and
nothing outside.  A 2-D H selects the shared call, a 3-D H the per-QP call the
shared one is held against (qpb_solve_box, qpb_solve_box_backward);
`host=True` the shared call's `_host` form on numpy buffers of the same kind.
The shared device calls also check that H's device buffer is bitwise unchanged.

The family: box_bwd_oracle.cycled(SEED, B, n) -- lb < 0 < ub, so every QP is
feasible -- with H[0] as the one H and the per-QP f, lb and ub.
"""
import ctypes
import math

import numpy as np

import box_bwd_oracle as BO
from box_bwd_oracle import NAMES
from bwd_harness import FILL8, GUARD, dev

SEED = 23
OUT = ("x", "lam", "active", "status", "iters")
FILL4 = np.frombuffer(bytes([0xA5] * 4), dtype=np.int32)[0]
DENSE_N, WAVE_N, GRAM_N = (1, 5, 16), (17, 20, 32), (33, 128)

_FAMILY = {}


def family(B, n):
    """(H0 (n,n), f, lb, ub (B,n)): computed once, shared, never modified."""
    if (B, n) not in _FAMILY:
        H, f, lb, ub, _ = BO.cycled(SEED, B, n)
        _FAMILY[(B, n)] = tuple(np.ascontiguousarray(a) for a in (H[0], f, lb, ub))
    return _FAMILY[(B, n)]


def batches_of(qpb, n):
    """shared_cases.batches, and 1 and 5 only at n = 128."""
    import shared_cases as SC
    return SC.batches(qpb)[:2] if n == 128 else SC.batches(qpb)


def same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


def bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _checked(k, raw, g, any_bits=False):
    """The guards of one flat buffer (numpy) are intact and every element between them was written."""
    raw, fill = (raw.view(np.int64), FILL8) if raw.dtype == np.float64 else (raw.view(np.int32), FILL4)
    assert (raw[:g] == fill).all() and (raw[-g:] == fill).all(), (k, "guard words written")
    if not any_bits:
        assert not (raw[g:-g] == fill).any(), (k, "elements never written")


def _p(t):
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr()) if hasattr(t, "data_ptr") else t.ctypes.data_as(ctypes.c_void_p)


def _buffers(spec, host):
    """{name: (flat buffer, guard, view of `count` elements)} filled with 0xA5; spec: {name: (count, numpy dtype)}."""
    import torch
    out = {}
    for k, (count, dt) in spec.items():
        if not count:
            continue
        g = GUARD * (8 // np.dtype(dt).itemsize)  # GUARD doubles either side
        if host:
            t = np.frombuffer(bytes([0xA5]) * ((count + 2 * g) * np.dtype(dt).itemsize), dtype=dt).copy()
        else:
            t = torch.empty(count + 2 * g, dtype=torch.float64 if dt == np.float64 else torch.int32, device="cuda")
            t.view(torch.uint8).fill_(0xA5)
        out[k] = (t, g, t[g:g + count])
    return out


def _collect(bufs, host, any_bits=()):
    out = {}
    for k, (t, g, view) in bufs.items():
        raw = t if host else t.cpu().numpy()
        _checked(k, raw, g, k in any_bits)
        out[k] = (view if host else view.cpu().numpy()).copy()
    return out


def solve(qpb, H, f, lb, ub, max_iter=0, stream=None, host=False):
    """H (n, n): qpb_solve_box_shared (host: its _host form); H (B, n, n):
    qpb_solve_box.  lb / ub may be None.  A dict of flat numpy outputs."""
    import torch
    B, n = f.shape
    m = 2 * n
    shared = H.ndim == 2
    assert shared or not host
    conv = (lambda a: None if a is None else np.ascontiguousarray(a)) if host else \
        (lambda a: None if a is None else dev(a))
    ins = [conv(a) for a in (H, f, lb, ub)]
    bufs = _buffers({"x": (B * n, np.float64), "lam": (B * m, np.float64), "active": (B * ((m + 31) // 32), np.int32),
                     "status": (B, np.int32), "iters": (B, np.int32)}, host)
    d = qpb.Desc(n, m, B, max_iter, 0, 0.0)
    args = [_p(t) for t in ins] + [_p(bufs[k][2]) for k in OUT]
    if host:
        rc = qpb.lib().qpb_solve_box_shared_host(ctypes.byref(d), *args)
    else:
        s = stream if stream is not None else torch.cuda.current_stream()
        fn = qpb.lib().qpb_solve_box_shared if shared else qpb.lib().qpb_solve_box
        rc = fn(ctypes.byref(d), *args, ctypes.c_void_p(s.cuda_stream))
    assert rc == 0, qpb.lib().qpb_last_error()
    if not host:
        s.synchronize()
        if shared:
            assert bits(ins[0].cpu().numpy(), np.ascontiguousarray(H)), "H was written"
    return _collect(bufs, host, any_bits=("active",))


def backward(qpb, H, x, act, st, g, need=NAMES, stream=None, host=False):
    """H (n, n): qpb_solve_box_shared_backward (host: its _host form), gH is
    (n, n); H (B, n, n): qpb_solve_box_backward.  st None: status NULL.  A dict
    of the numpy outputs in `need`."""
    import torch
    Bq, n = g.shape
    shared = H.ndim == 2
    assert shared or not host
    conv = (lambda a: None if a is None else np.ascontiguousarray(a)) if host else \
        (lambda a: None if a is None else dev(a))
    ins = [conv(a) for a in (H, x, act, st, g)]
    shp = {"H": H.shape, "f": (Bq, n), "lb": (Bq, n), "ub": (Bq, n)}
    bufs = _buffers({k: (math.prod(shp[k]), np.float64) for k in NAMES if k in need}, host)
    d = qpb.Desc(n, 2 * n, Bq, 0, 0, 0.0)
    args = [_p(t) for t in ins] + [_p(bufs[k][2]) if k in bufs else None for k in NAMES]
    if host:
        rc = qpb.lib().qpb_solve_box_shared_backward_host(ctypes.byref(d), *args)
    else:
        s = stream if stream is not None else torch.cuda.current_stream()
        fn = qpb.lib().qpb_solve_box_shared_backward if shared else qpb.lib().qpb_solve_box_backward
        rc = fn(ctypes.byref(d), *args, ctypes.c_void_p(s.cuda_stream))
    assert rc == 0, qpb.lib().qpb_last_error()
    if not host:
        s.synchronize()
        if shared:
            assert bits(ins[0].cpu().numpy(), np.ascontiguousarray(H)), "H was written"
    out = _collect(bufs, host)
    return {k: v.reshape(shp[k]) for k, v in out.items()}
