"""TEST INFRASTRUCTURE ONLY: what the tests of qpb_factor_box /
qpb_solve_box_factored share (tests/test_gpu_box_factored*.py), in
tests/factored_cases.py's manner.

The inputs are tests/box_shared_harness.family(B, n) -- ONE H0, f, lb < 0 < ub
per QP -- at n in NS (gi_box padded and N16, gi_wave's BOX form) and the batches
1, 5 and 67: a single QP, a ragged group of four, several wavefronts with a
ragged tail.

`oracle` solves a case once on the CPU (box_bwd_oracle.solve) and says which
QPs are strictly complementary: the only ones on which two correct solvers must
agree on the active set.

`factor` and `solve` call qpb_factor_box and qpb_solve_box_factored through the
C-ABI into buffers filled with 0xA5 and fenced by guard words, and check that
every element was written and nothing outside; `host=True` the `_host` forms on
numpy buffers of the same kind.
"""
import ctypes

import numpy as np

import box_bwd_oracle as BO
import box_shared_harness as BH
from bwd_harness import FILL8, GUARD, dev

NS = (1, 5, 16, 17, 20, 32)
BATCHES = (1, 5, 67)
X_TOL, LAM_TOL, KKT_TOL = 1e-6, 1e-6, 1e-9  # test_gpu_box.py's bars, the ones qpb_solve_box is held to
STRICT = 1e-8                               # strict complementarity: margin over the scale
MIN_STRICT_SHARE = 0.95                     # a condition on the inputs, not a measurement
OUT = ("x", "lam", "active", "status", "iters")
FILL4 = BH.FILL4

_ORACLE = {}


def oracle(B, n):
    """(x (B,n), lam (B,2n), active (B,2n) bool, strict (B,) bool) of
    BH.family(B, n): computed once, shared, never modified.  strict: the smallest
    multiplier on an active bound exceeds STRICT (1 + max|lam|) and the smallest
    slack on an inactive one exceeds STRICT (1 + max|b| + max|x|)."""
    if (B, n) not in _ORACLE:
        H0, f, lb, ub = BH.family(B, n)
        x, lam, act = BO.solve(np.broadcast_to(H0, (B, n, n)), f, lb, ub)
        act = np.asarray(act, bool)
        b = np.concatenate([ub, -lb], axis=1)
        slack = b - np.concatenate([x, -x], axis=1)
        ln = 1.0 + np.abs(lam).max(axis=1)
        sc = 1.0 + np.abs(b).max(axis=1) + np.abs(x).max(axis=1)
        lmin = np.where(act, lam, np.inf).min(axis=1)
        smin = np.where(~act, slack, np.inf).min(axis=1)
        _ORACLE[(B, n)] = (x, lam, act, (lmin > STRICT * ln) & (smin > STRICT * sc))
    return _ORACLE[(B, n)]


def relx(x, xr):
    return np.abs(x - xr).max(axis=1) / np.maximum(1.0, np.abs(xr).max(axis=1))


def rell(lam, lr):
    return np.abs(lam - lr).max(axis=1) / (1.0 + np.abs(lr).max(axis=1))


def mask_of(active, n):
    """(B, 2n) bool from the (B, ceil(2n/32)) words."""
    w = active.reshape(len(active), -1).view(np.uint32)
    rows = np.arange(2 * n)
    return ((w[:, rows // 32] >> (rows % 32).astype(np.uint32)) & 1).astype(bool)


def kkt(H0, f, lb, ub, x, lam):
    """The worst of oracle.kkt_residuals over the batch, absent bounds (NaN, +-inf) left out."""
    B, n = f.shape
    ub = np.full((B, n), np.inf) if ub is None else ub
    lb = np.full((B, n), -np.inf) if lb is None else lb
    b = np.concatenate([ub, -lb], axis=1)
    fin = np.isfinite(b)
    A, _ = BO.dense(np.zeros((B, n)), np.zeros((B, n)))
    A = A * fin[:, :, None]
    r = BO.O.kkt_residuals(np.broadcast_to(H0, (B, n, n)), f, A, np.where(fin, b, 0.0), x, lam)
    return max(float(v.max()) for v in r.values())


def _guarded(torch, count, dt, host):
    g = GUARD * (2 if dt == np.int32 else 1)  # GUARD doubles either side
    if host:
        return np.frombuffer(bytes([0xA5]) * ((count + 2 * g) * np.dtype(dt).itemsize), dtype=dt).copy(), g
    t = torch.empty(count + 2 * g, dtype=torch.float64 if dt == np.float64 else torch.int32, device="cuda")
    t.view(torch.uint8).fill_(0xA5)
    return t, g


def _checked(t, g, name, all_written=True):
    raw = t if isinstance(t, np.ndarray) else t.cpu().numpy()
    words, fill = (raw.view(np.int64), FILL8) if raw.dtype == np.float64 else (raw, FILL4)
    assert (words[:g] == fill).all() and (words[-g:] == fill).all(), (name, "guard words written")
    if all_written:
        assert not (words[g:-g] == fill).any(), (name, "elements never written")
    return raw[g:len(raw) - g].copy()


def _ptr(t, off=0):
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        return ctypes.c_void_p(t.ctypes.data + off * t.itemsize)
    return ctypes.c_void_p(t.data_ptr() + off * t.element_size())


def _sp(torch, stream):
    s = stream if stream is not None else torch.cuda.current_stream()
    return s, ctypes.c_void_p(s.cuda_stream)


def factor(qpb, H0, stream=None, sync=True, host=False, fstatus=True):
    """qpb_factor_box on numpy H0 (n, n): (bxfac buffer, its guard offset, fstatus
    buffer or None, its guard offset, H on the device) -- device tensors, so that
    a solve can be queued behind the factorisation without a host
    synchronisation; `factor_result` reads them back and checks them."""
    import torch
    n = H0.shape[0]
    k = qpb.lib().qpb_factor_box_doubles(n)
    assert k == qpb.factor_box_doubles(n) and k > 0
    if host:
        ft, fg = _guarded(torch, k, np.float64, host)
        st, sg = _guarded(torch, 1, np.int32, host) if fstatus else (None, 0)
        H = np.ascontiguousarray(H0)
        rc = qpb.lib().qpb_factor_box_host(n, _ptr(H), _ptr(ft, fg), _ptr(st, sg))
        assert rc == 0, qpb.lib().qpb_last_error()
        return ft, fg, st, sg, H
    s, sp = _sp(torch, stream)
    with torch.cuda.stream(s):  # the buffers' fill and H's upload precede the launch on its own stream
        ft, fg = _guarded(torch, k, np.float64, host)
        st, sg = _guarded(torch, 1, np.int32, host) if fstatus else (None, 0)
        H = dev(H0)
    rc = qpb.lib().qpb_factor_box(n, _ptr(H), _ptr(ft, fg), _ptr(st, sg), sp)
    assert rc == 0, qpb.lib().qpb_last_error()
    if sync:
        s.synchronize()
        assert BH.bits(H.cpu().numpy(), np.ascontiguousarray(H0)), "H was written"
    return ft, fg, st, sg, H


def factor_result(F):
    """(bxfac numpy, fstatus int or None) of `factor`'s result, guards and coverage checked."""
    ft, fg, st, sg, _ = F
    return _checked(ft, fg, "bxfac"), (None if st is None else int(_checked(st, sg, "fstatus")[0]))


def solve(qpb, F, f, lb, ub, max_iter=0, stream=None, iters=True, host=False):
    """qpb_solve_box_factored on `factor`'s result and f, lb, ub (B, n) -- numpy, or
    CUDA tensors; lb / ub may be None -- into guarded buffers; a dict of numpy
    outputs (without "iters" when iters is False: the pointer is NULL)."""
    import torch
    ft, fg = F[0], F[1]
    B, n = f.shape
    m, w = 2 * n, (2 * n + 31) // 32
    spec = {"x": (B * n, np.float64), "lam": (B * m, np.float64), "active": (B * w, np.int32),
            "status": (B, np.int32), "iters": (B if iters else 0, np.int32)}
    d = qpb.Desc(n, m, B, max_iter, 0, 0.0)
    if host:
        bufs = {k: _guarded(torch, c, dt, host) for k, (c, dt) in spec.items() if c}
        outs = [_ptr(*bufs[k]) if k in bufs else None for k in OUT]
        ins = [None if a is None else np.ascontiguousarray(a) for a in (f, lb, ub)]
        rc = qpb.lib().qpb_solve_box_factored_host(ctypes.byref(d), _ptr(ft, fg), *[_ptr(a) for a in ins], *outs)
        assert rc == 0, qpb.lib().qpb_last_error()
    else:
        s, sp = _sp(torch, stream)
        with torch.cuda.stream(s):
            # (tensors are taken as they are: uploaded before the work they must not wait for)
            ins = [None if a is None else a if torch.is_tensor(a) else dev(a) for a in (f, lb, ub)]
            bufs = {k: _guarded(torch, c, dt, host) for k, (c, dt) in spec.items() if c}  # filled on the launch's stream
        outs = [_ptr(*bufs[k]) if k in bufs else None for k in OUT]
        rc = qpb.lib().qpb_solve_box_factored(ctypes.byref(d), _ptr(ft, fg), *[_ptr(a) for a in ins], *outs, sp)
        assert rc == 0, qpb.lib().qpb_last_error()
        s.synchronize()
    out = {k: _checked(t, g, k, all_written=k != "active") for k, (t, g) in bufs.items()}  # (a mask may hold any bits)
    out["x"] = out["x"].reshape(B, n)
    out["lam"] = out["lam"].reshape(B, m)
    out["active"] = out["active"].reshape(B, w)
    return out


def shared(qpb, H0, f, lb, ub, max_iter=0):
    """qpb_solve_box_shared on the same inputs: the unfactored path (box_shared_harness.solve)."""
    out = BH.solve(qpb, np.ascontiguousarray(H0), f, lb, ub, max_iter=max_iter)
    B, n = f.shape
    out["x"] = out["x"].reshape(B, n)
    out["lam"] = out["lam"].reshape(B, 2 * n)
    out["active"] = out["active"].reshape(B, -1)
    return out
