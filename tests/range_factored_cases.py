"""TEST INFRASTRUCTURE ONLY: what the tests of qpb_solve_range_factored share
(tests/test_gpu_range_factored*.py, tests/test_range_factored_cases.py).

The inputs are tests/shared_cases.py's family -- ONE H0 and ONE A0, f and b per
QP -- made two-sided: bu = b, and bl = A0 xc - 10 U(0.1, 1) with
bl[:, :meq] = bu[:, :meq], xc the family's own strictly feasible point, so every
QP keeps a slack of at least 1 on both sides.  The shapes are SC.SHAPES and
(16, 16, 3), the n = 16, m = 16 form with one row of D per lane; the batches are
1, 5 and 67.

`oracle` solves a case once on the CPU (range_oracle.range_solve per QP) and
says which QPs are strictly complementary: the only ones on which two correct
solvers must agree on `active` and `lower`.

`solve` calls qpb_solve_range_factored through the C-ABI on factored_cases'
`factor` result, into buffers filled with 0xA5 and fenced by guard words, and
checks that every element was written and nothing outside.  `unfactored` is
qpb_solve_range(shared = H | A) on the same inputs.
"""
import ctypes

import numpy as np

import eq_oracle as EO
import factored_cases as FC
import range_oracle as RO
import shared_cases as SC
from bwd_harness import dev

BATCHES = (1, 5, 67)
FULL_MR1 = (16, 16, 3)
SHAPES = list(SC.SHAPES) + [FULL_MR1]
ROW_SHAPES = [s for s in SHAPES if s[1] > 0]
X_TOL, LAM_TOL, KKT_TOL = 1e-6, 1e-6, 1e-9  # test_gpu_range.py's bars, the ones qpb_solve_range is held to
STRICT = 1e-8                               # strict complementarity: margin over the scale
MIN_STRICT_SHARE = 0.95                     # a condition on the inputs, not a measurement
MIN_SIDE_SHARE = 0.25                       # ... at B = 67: each side's share of the active inequality rows
OUT = ("x", "lam", "active", "lower", "status", "iters")

_FAMILY, _ORACLE = {}, {}


def family(B, n, m, meq):
    """(H0 (n,n), f (B,n), A0 (m,n), bl (B,m), bu (B,m), xc (B,n)): computed once, shared, never modified."""
    key = (B, n, m, meq)
    if key not in _FAMILY:
        H0, f, A0, b = SC.family(B, n, m, meq)
        if m == 0:
            _FAMILY[key] = (H0, f, A0, np.zeros((B, 0)), b, np.zeros((B, n)))
        else:
            xc = EO.eq_family(SC.SEED, B, n, m, meq)[4]
            rng = np.random.default_rng([SC.SEED, n, m, meq, 0x7A9E])
            bl = xc @ A0.T - 10.0 * rng.uniform(0.1, 1.0, size=b.shape)
            bl[:, :meq] = b[:, :meq]
            _FAMILY[key] = (H0, f, A0, bl, b, xc)
    return _FAMILY[key]


def oracle(B, n, m, meq):
    """(x (B,n), lam (B,m) signed, active (B,m) bool, lower (B,m) bool, strict (B,) bool,
    status (B,)) of `family`: computed once, shared, never modified.  strict: on
    the rows >= meq the smallest |multiplier| of an active row exceeds
    STRICT (1 + max|lam|), and the smaller of an inactive row's two slacks exceeds
    STRICT times the primal scale 1 + max(|bu|, |bl|) + |A|_inf max|x|."""
    key = (B, n, m, meq)
    if key not in _ORACLE:
        H0, f, A0, bl, bu, xc = family(B, n, m, meq)
        if m == 0:
            x = np.linalg.solve(H0, -f.T).T
            _ORACLE[key] = (x, np.zeros((B, 0)), np.zeros((B, 0), bool), np.zeros((B, 0), bool), np.ones(B, bool),
                            np.zeros(B, int))
        else:
            refs = [RO.range_solve(H0, f[i], A0, bl[i], bu[i], meq, xc[i]) for i in range(B)]
            x = np.array([r.x for r in refs])
            lam = np.array([r.lam for r in refs])
            act = np.array([r.active for r in refs], bool)
            low = np.array([r.lower for r in refs], bool)
            ax = x @ A0.T
            slack = np.minimum(bu - ax, ax - bl)
            ln = 1.0 + np.abs(lam).max(axis=1)
            sc = (1.0 + np.maximum(np.abs(bu).max(axis=1), np.abs(bl[:, meq:]).max(axis=1, initial=0.0))
                  + np.abs(A0).sum(axis=1).max() * np.abs(x).max(axis=1))
            ineq = np.arange(m) >= meq
            lmin = np.where(act & ineq, np.abs(lam), np.inf).min(axis=1)
            smin = np.where(~act & ineq, slack, np.inf).min(axis=1)
            _ORACLE[key] = (x, lam, act, low, (lmin > STRICT * ln) & (smin > STRICT * sc),
                            np.array([r.status for r in refs]))
    return _ORACLE[key]


def kkt(H0, f, A0, bl, bu, meq, x, lam):
    """range_oracle.kkt_range's worst residuals over the batch, H0 and A0 shared."""
    B = len(f)
    res = RO.kkt_range(SC.expand(H0, B), f, SC.expand(A0, B), bl, bu, meq, x, lam)
    return {k: float(v.max()) for k, v in res.items()}


def solve(qpb, F, f, bl, bu, meq, max_iter=0, stream=None, iters=True, lower=True):
    """qpb_solve_range_factored on factored_cases.factor's result and f (B, n), bl
    and bu (B, m; either may be None) -- numpy, or CUDA tensors -- into guarded
    buffers; a dict of numpy outputs (without "iters" / "lower" where that
    pointer is NULL)."""
    import torch
    ft, fg = F[0], F[1]
    B, n = f.shape
    some = bu if bu is not None else bl
    m = 0 if some is None else some.shape[1]
    w = (m + 31) // 32
    spec = {"x": (B * n, torch.float64), "lam": (B * m, torch.float64), "active": (B * w, torch.int32),
            "lower": (B * w if lower else 0, torch.int32), "status": (B, torch.int32),
            "iters": (B if iters else 0, torch.int32)}
    bufs = {k: FC._guarded(torch, c, dt) for k, (c, dt) in spec.items() if c}
    ptr = lambda k: ctypes.c_void_p(bufs[k][0][bufs[k][1]:].data_ptr()) if k in bufs else None  # noqa: E731
    s, sp = FC._sp(torch, stream)
    with torch.cuda.stream(s):
        up = lambda a: None if a is None or not m else (a if torch.is_tensor(a) else dev(a))  # noqa: E731
        fd = f if torch.is_tensor(f) else dev(f)
        bld, bud = up(bl), up(bu)
    d = qpb.Desc(n, m, B, max_iter, 0, 0.0)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    rc = qpb.lib().qpb_solve_range_factored(ctypes.byref(d), meq, ctypes.c_void_p(ft[fg:].data_ptr()), p(fd), p(bld),
                                            p(bud), *[ptr(k) for k in OUT], sp)
    assert rc == 0, qpb.lib().qpb_last_error()
    s.synchronize()
    # (a mask may hold any bits)
    out = {k: FC._checked(t, g, k, all_written=k not in ("active", "lower")) for k, (t, g) in bufs.items()}
    out["x"] = out["x"].reshape(B, n)
    out["lam"] = out["lam"].reshape(B, m) if m else np.zeros((B, 0))
    out["active"] = out["active"].reshape(B, w) if m else np.zeros((B, 0), np.int32)
    if lower:
        out["lower"] = out["lower"].reshape(B, w) if m else np.zeros((B, 0), np.int32)
    return out


def unfactored(qpb, H0, f, A0, bl, bu, meq, max_iter=0):
    """qpb_solve_range(shared = H | A) on the same inputs: the unfactored path (m > 0)."""
    import torch
    sol = qpb.solve_range(dev(H0), dev(f), dev(A0), None if bl is None else dev(bl), None if bu is None else dev(bu),
                          meq, max_iter=max_iter)
    torch.cuda.synchronize()
    return {k: getattr(sol, k).cpu().numpy() for k in OUT}
