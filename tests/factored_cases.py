"""TEST INFRASTRUCTURE ONLY: what the tests of qpb_factor_shared /
qpb_solve_factored share (tests/test_gpu_factored*.py, tests/test_factored_cases.py).

The inputs are tests/shared_cases.py's family -- ONE H0 and ONE A0, f and b per
QP, every QP strictly feasible -- at its SHAPES and the batches 1, 5 and 67:
every load path of the n <= 16 kernel, a ragged group of four, both classes.

`oracle` solves a case once on the CPU (eq_oracle.eq_solve from the family's
own strictly feasible point) and says which QPs are strictly complementary:
the only ones on which two correct solvers must agree on the active set.

`factor` and `solve` call qpb_factor_shared and qpb_solve_factored through the
C-ABI into buffers filled with 0xA5 and fenced by guard words (the helpers of
tests/bwd_harness.py), and check that every element was written and nothing
outside.
"""
import ctypes

import numpy as np

import eq_oracle as EO
import shared_cases as SC
from bwd_harness import FILL8, GUARD, dev

BATCHES = (1, 5, 67)
SHAPES = SC.SHAPES
X_TOL, LAM_TOL, KKT_TOL = 1e-6, 1e-6, 1e-9  # test_gpu_eq.py's bars, the ones qpb_solve_eq is held to
STRICT = 1e-8                               # strict complementarity: margin over the scale
MIN_STRICT_SHARE = 0.95                     # a condition on the inputs, not a measurement
OUT = ("x", "lam", "active", "status", "iters")
FILL4 = np.frombuffer(bytes([0xA5] * 4), dtype=np.int32)[0]

_ORACLE = {}


def oracle(B, n, m, meq):
    """(x (B,n), lam (B,m), active (B,m) bool, strict (B,) bool) of
    SC.family(B, n, m, meq): computed once, shared, never modified.  strict: the
    smallest multiplier on an active inequality exceeds STRICT (1 + max|lam|)
    and the smallest slack on an inactive row exceeds STRICT times the primal
    scale of eq_oracle.kkt_mixed, 1 + max|b| + |A|_inf max|x|."""
    key = (B, n, m, meq)
    if key not in _ORACLE:
        H0, f, A0, b = SC.family(B, n, m, meq)
        if m == 0:
            x = np.linalg.solve(H0, -f.T).T
            _ORACLE[key] = (x, np.zeros((B, 0)), np.zeros((B, 0), bool), np.ones(B, bool))
        else:
            xc = EO.eq_family(SC.SEED, B, n, m, meq)[4]
            refs = [EO.eq_solve(H0, f[i], A0, b[i], meq, xc[i]) for i in range(B)]
            assert all(r.status == 0 for r in refs), key
            x = np.array([r.x for r in refs])
            lam = np.array([r.lam for r in refs])
            act = np.array([r.active for r in refs], bool)
            slack = b - x @ A0.T
            ln = 1.0 + np.abs(lam).max(axis=1)
            sc = 1.0 + np.abs(b).max(axis=1) + np.abs(A0).sum(axis=1).max() * np.abs(x).max(axis=1)
            ineq = np.arange(m) >= meq
            lmin = np.where(act & ineq, lam, np.inf).min(axis=1)
            smin = np.where(~act & ineq, slack, np.inf).min(axis=1)
            _ORACLE[key] = (x, lam, act, (lmin > STRICT * ln) & (smin > STRICT * sc))
    return _ORACLE[key]


def relx(x, xr):
    return np.abs(x - xr).max(axis=1) / np.maximum(1.0, np.abs(xr).max(axis=1))


def rell(lam, lr):
    return np.abs(lam - lr).max(axis=1) / (1.0 + np.abs(lr).max(axis=1)) if lam.shape[1] else np.zeros(len(lam))


def _guarded(torch, count, dt):
    g = GUARD * (2 if dt == torch.int32 else 1)  # GUARD doubles either side
    t = torch.empty(count + 2 * g, dtype=dt, device="cuda")
    t.view(torch.uint8).fill_(0xA5)
    return t, g


def _checked(t, g, name, all_written=True):
    raw = t.cpu().numpy()
    raw, fill = (raw.view(np.int64), FILL8) if raw.dtype == np.float64 else (raw, FILL4)
    assert (raw[:g] == fill).all() and (raw[-g:] == fill).all(), (name, "guard words written")
    if all_written:
        assert not (raw[g:-g] == fill).any(), (name, "elements never written")
    return t[g:t.numel() - g].cpu().numpy()


def _sp(torch, stream):
    s = stream if stream is not None else torch.cuda.current_stream()
    return s, ctypes.c_void_p(s.cuda_stream)


def factor(qpb, H0, A0, stream=None, sync=True):
    """qpb_factor_shared on numpy H0 (n, n) and A0 (m, n): (fac tensor, its guard
    offset, fstatus tensor, its guard offset) -- device tensors, so that a solve
    can be queued behind the factorisation without a host synchronisation;
    `factor_result` reads them back and checks them."""
    import torch
    n, m = H0.shape[0], A0.shape[0]
    k = qpb.lib().qpb_factor_doubles(n, m)
    assert k == qpb.factor_doubles(n, m) and k > 0
    ft, fg = _guarded(torch, k, torch.float64)
    st, sg = _guarded(torch, 1, torch.int32)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    s, sp = _sp(torch, stream)
    with torch.cuda.stream(s):
        H, A = dev(H0), dev(A0) if m else None
    rc = qpb.lib().qpb_factor_shared(n, m, ptr(H), ptr(A), ptr(ft[fg:]), ptr(st[sg:]), sp)
    assert rc == 0, qpb.lib().qpb_last_error()
    if sync:
        s.synchronize()
    return ft, fg, st, sg, (H, A)


def factor_result(F):
    """(fac numpy, fstatus int) of `factor`'s result, guards and coverage checked."""
    ft, fg, st, sg, _ = F
    return _checked(ft, fg, "fac"), int(_checked(st, sg, "fstatus")[0])


def solve(qpb, F, f, b, meq, max_iter=0, stream=None, iters=True):
    """qpb_solve_factored on `factor`'s result and f (B, n), b (B, m) -- numpy, or
    CUDA tensors -- into guarded buffers; a dict of numpy outputs (without "iters" when iters is
    False: the pointer is NULL)."""
    import torch
    ft, fg = F[0], F[1]
    B, n = f.shape
    m = 0 if b is None else b.shape[1]
    w = (m + 31) // 32
    spec = {"x": (B * n, torch.float64), "lam": (B * m, torch.float64), "active": (B * w, torch.int32),
            "status": (B, torch.int32), "iters": (B if iters else 0, torch.int32)}
    bufs = {k: _guarded(torch, c, dt) for k, (c, dt) in spec.items() if c}
    ptr = lambda k: ctypes.c_void_p(bufs[k][0][bufs[k][1]:].data_ptr()) if k in bufs else None  # noqa: E731
    s, sp = _sp(torch, stream)
    with torch.cuda.stream(s):
        # (tensors are taken as they are: uploaded before the work they must not wait for)
        fd = f if torch.is_tensor(f) else dev(f)
        bd = (b if torch.is_tensor(b) else dev(b)) if m else None
    d = qpb.Desc(n, m, B, max_iter, 0, 0.0)
    rc = qpb.lib().qpb_solve_factored(ctypes.byref(d), meq, ctypes.c_void_p(ft[fg:].data_ptr()),
                                      ctypes.c_void_p(fd.data_ptr()), ctypes.c_void_p(bd.data_ptr()) if m else None,
                                      *[ptr(k) for k in OUT], sp)
    assert rc == 0, qpb.lib().qpb_last_error()
    s.synchronize()
    out = {k: _checked(t, g, k, all_written=k != "active") for k, (t, g) in bufs.items()}  # (a mask may hold any bits)
    out["x"] = out["x"].reshape(B, n)
    out["lam"] = out["lam"].reshape(B, m) if m else np.zeros((B, 0))
    out["active"] = out["active"].reshape(B, w) if m else np.zeros((B, 0), np.int32)
    return out


def shared(qpb, H0, f, A0, b, meq, max_iter=0):
    """qpb_solve_shared(shared = H | A) on the same inputs: the unfactored path."""
    import torch
    m = A0.shape[0]
    sol = qpb.solve_shared(dev(H0), dev(f), dev(A0) if m else None, dev(b) if m else None, meq, max_iter=max_iter)
    torch.cuda.synchronize()
    out = {k: getattr(sol, k).cpu().numpy() for k in OUT}
    if not m:
        out["lam"] = np.zeros((len(f), 0))
    return out
