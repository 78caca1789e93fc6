"""TEST INFRASTRUCTURE ONLY: the oracle for qpb_solve_backward (numpy, no GPU).

For one solved QP with active set W (a boolean mask over the m rows), the
gradients of a loss l(x) with respect to (H, f, A, b) given g = dl/dx follow
from the KKT system at fixed active set,

    [ H    A_W^T ] [ dx   ]     [ g ]
    [ A_W   0    ] [ dlam ] = - [ 0 ]

    dl/df = dx                        dl/dH   = 1/2 (dx x^T + x dx^T)
    dl/db_i = -dlam_i                 dl/dA_i = dlam_i x^T + lam_i dx^T   (i in W, else 0)

`backward` solves the dense system with numpy.linalg.solve (A_W must have full
row rank); `certificate` measures how well a set of OUTPUTS satisfies the
system, without solving anything.
"""
from __future__ import annotations

import numpy as np

import eq_oracle as EO


def family(seed: int, count: int, n: int, m: int, meq: int):
    """eq_oracle.eq_family, and at m = 0 (which it has no form for) its H and
    f with an A of no rows.  Returns (H, f, A, b, xc)."""
    if m > 0:
        return EO.eq_family(seed, count, n, m, meq)
    H, f, A, b, xc = EO.eq_family(seed, count, n, 1, 0)
    return H, f, A[:, :0], b[:, :0], xc


def backward(H, x, lam, A, act, g):
    """One QP: (gH, gf, gA, gb).  A is (m, n) (m may be 0), act a bool mask (m,)."""
    H, x, g = (np.asarray(v, float) for v in (H, x, g))
    n = H.shape[0]
    A = np.zeros((0, n)) if A is None else np.asarray(A, float).reshape(-1, n)
    m = A.shape[0]
    lam = np.zeros(m) if lam is None else np.asarray(lam, float)
    W = np.flatnonzero(np.asarray(act, bool)) if m else np.zeros(0, int)
    k = len(W)
    K = np.zeros((n + k, n + k))
    K[:n, :n] = H
    K[:n, n:] = A[W].T
    K[n:, :n] = A[W]
    sol = np.linalg.solve(K, -np.concatenate([g, np.zeros(k)]))
    dx, dl = sol[:n], sol[n:]
    gA = np.zeros((m, n))
    gb = np.zeros(m)
    gA[W] = np.outer(dl, x) + np.outer(lam[W], dx)
    gb[W] = -dl
    gH = 0.5 * (np.outer(dx, x) + np.outer(x, dx))
    return gH, dx.copy(), gA, gb


def certificate(H, A, act, g, gf, gb):
    """The two relative residuals of one QP's backward system from the outputs
    alone, with dx = gf and dlam_W = -gb_W:
        |H dx + A_W^T dlam + g|_inf / (1 + |g|_inf + ||H||_inf |dx|_inf)
        |A_W dx|_inf / (1 + ||A||_inf |dx|_inf)"""
    H, g, dx = (np.asarray(v, float) for v in (H, g, gf))
    n = H.shape[0]
    A = np.zeros((0, n)) if A is None else np.asarray(A, float).reshape(-1, n)
    m = A.shape[0]
    W = np.flatnonzero(np.asarray(act, bool)) if m else np.zeros(0, int)
    dl = -np.asarray(gb, float)[W] if m else np.zeros(0)
    dxn = np.abs(dx).max()
    r1 = H @ dx + A[W].T @ dl + g
    stat = np.abs(r1).max() / (1.0 + np.abs(g).max() + np.abs(H).sum(axis=1).max() * dxn)
    r2 = A[W] @ dx
    An = np.abs(A).sum(axis=1).max() if m else 0.0
    prim = (np.abs(r2).max() if len(W) else 0.0) / (1.0 + An * dxn)
    return float(stat), float(prim)
