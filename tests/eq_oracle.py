"""TEST INFRASTRUCTURE ONLY: the oracle for qpb_solve_eq (numpy, no GPU).

    min 1/2 x^T H x + f^T x   s.t.   E x = d,  G x <= h
    with A = [E; G], b = [d; h], E = A[:meq]  (qpb.h's row order)

The kernels take the equalities natively (Goldfarb-Idnani); the oracle does
not.  It removes them by a null-space reduction and hands what is left to the
unchanged primal active-set solver of oracle/oracle.py: from a point xc with
E xc = d and G xc < h, write x = xc + Z y with the columns of Z a basis of
null(E) (the last n - meq columns of a complete QR of E^T) and solve

    min 1/2 y^T (Z^T H Z) y + (Z^T (H xc + f))^T y   s.t.   (G Z) y <= h - G xc

from y = 0.  The inequality multipliers are the reduced problem's; the
equality multipliers follow from stationarity, E^T lam_eq = -(H x + f + G^T
lam_in), by least squares (E has full row rank here).  meq = n leaves no y:
x = xc (the oracle rejects the empty reshape), no inequality active.
"""
from __future__ import annotations

import numpy as np

import oracle as O


def eq_family(seed: int, count: int, n: int, m: int, meq: int):
    """oracle.family_shifted with the first meq rows made equalities through
    xc: b[:, :meq] = A[:, :meq] xc.  xc satisfies them and is strictly feasible
    for the rest (slack >= 1).  Returns (H, f, A, b, xc)."""
    H, f, A, b, xc = O.family_shifted(seed, count, n, m)
    b[:, :meq] = np.einsum("bij,bj->bi", A[:, :meq], xc)
    return H, f, A, b, xc


def eq_solve(H, f, A, b, meq: int, xc) -> O.ASResult:
    """One QP; E = A[:meq] must have full row rank (meq <= n).  The result's
    lam and active cover all m rows (active[:meq] all set)."""
    H, f, A, b, xc = (np.asarray(v, float) for v in (H, f, A, b, xc))
    n, m = H.shape[0], A.shape[0]
    if meq == 0:
        return O.active_set_solve(H, f, A, b, x0=xc)
    assert meq <= n and meq <= m
    E, G, h = A[:meq], A[meq:], b[meq:]
    Q, _ = np.linalg.qr(E.T, mode="complete")
    Z = Q[:, meq:]
    lam = np.zeros(m)
    act = np.zeros(m, bool)
    act[:meq] = True
    iters, status = 0, 0
    if Z.shape[1] == 0:
        x = xc.copy()
    else:
        r = O.active_set_solve(Z.T @ H @ Z, Z.T @ (H @ xc + f), G @ Z, h - G @ xc, x0=np.zeros(n - meq))
        x = xc + Z @ r.x
        lam[meq:], act[meq:], iters, status = r.lam, r.active, r.iters, r.status
    lam[:meq] = np.linalg.lstsq(E.T, -(H @ x + f + G.T @ lam[meq:]), rcond=None)[0]
    return O.ASResult(x, lam, act, iters, status)


def kkt_mixed(H, f, A, b, meq: int, x, lam):
    """oracle.kkt_residuals for rows 0 .. meq-1 equalities: the same four
    relative residuals on the same four scales.  The equality residual
    |E x - d| joins the violation in `prim`; `dual` and `comp` run over the
    rows >= meq only (an equality's multiplier is free and its slack is its
    residual)."""
    H, f, A, b, x, lam = (np.asarray(v, float) for v in (H, f, A, b, x, lam))
    r = np.einsum("bij,bj->bi", H, x) + f + np.einsum("bij,bi->bj", A, lam)
    xn = np.abs(x).max(axis=1)
    Hn = np.abs(H).sum(axis=2).max(axis=1)
    stat = np.abs(r).max(axis=1) / (1.0 + np.abs(f).max(axis=1) + Hn * xn)
    An = np.abs(A).sum(axis=2).max(axis=1)
    sc = 1.0 + np.abs(b).max(axis=1) + An * xn
    slack = b - np.einsum("bij,bj->bi", A, x)
    z = np.zeros(len(x))
    viol = np.maximum(0.0, -slack[:, meq:].min(axis=1)) if meq < A.shape[1] else z
    res = np.abs(slack[:, :meq]).max(axis=1) if meq else z
    prim = np.maximum(viol, res) / sc
    ln = 1.0 + np.abs(lam).max(axis=1)
    if meq < A.shape[1]:
        dual = np.maximum(0.0, -lam[:, meq:].min(axis=1)) / ln
        comp = np.abs(lam[:, meq:] * slack[:, meq:]).max(axis=1) / (ln * sc)
    else:
        dual, comp = z, z
    return {"stat": stat, "prim": prim, "dual": dual, "comp": comp}


_CACHE = {}


def eq_reference(seed: int, count: int, n: int, m: int, meq: int):
    """(H, f, A, b, xc, refs) of eq_family, solved once per session and shared
    (never modified) by the tests that need it."""
    key = (seed, count, n, m, meq)
    if key not in _CACHE:
        H, f, A, b, xc = eq_family(seed, count, n, m, meq)
        refs = [eq_solve(H[i], f[i], A[i], b[i], meq, xc[i]) for i in range(count)]
        assert all(r.status == 0 for r in refs), key
        _CACHE[key] = (H, f, A, b, xc, refs)
    return _CACHE[key]
