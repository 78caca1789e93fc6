"""TEST INFRASTRUCTURE ONLY: the oracle for qpb_solve_backward_dual (numpy, no GPU).

For one solved QP with active set W and a loss l(x, lam), g = dl/dx and
glam = dl/dlam, the gradients follow from the KKT system of tests/kkt_oracle.py
with a full right-hand side,

    [ H    A_W^T ] [ dx   ]     [ g      ]
    [ A_W   0    ] [ dlam ] = - [ glam_W ]

and its output formulas, unchanged.  `backward` solves the dense system with
numpy.linalg.solve (A_W must have full row rank); `certificate` measures how
well a set of OUTPUTS satisfies it; `tangent` is the same solve read as the
forward sensitivity of (x*, lam*) along (df, db).
"""
from __future__ import annotations

import numpy as np


def _system(H, A, act):
    H = np.asarray(H, float)
    n = H.shape[0]
    A = np.zeros((0, n)) if A is None else np.asarray(A, float).reshape(-1, n)
    m = A.shape[0]
    W = np.flatnonzero(np.asarray(act, bool)) if m else np.zeros(0, int)
    k = len(W)
    K = np.zeros((n + k, n + k))
    K[:n, :n] = H
    K[:n, n:] = A[W].T
    K[n:, :n] = A[W]
    return H, A, W, K


def backward(H, x, lam, A, act, g, glam):
    """One QP: (gH, gf, gA, gb).  A is (m, n) (m may be 0), act a bool mask (m,),
    glam (m,) -- its entries outside W are never read."""
    H, A, W, K = _system(H, A, act)
    x, g = np.asarray(x, float), np.asarray(g, float)
    n, m, k = H.shape[0], A.shape[0], len(W)
    lam = np.zeros(m) if lam is None else np.asarray(lam, float)
    glw = np.asarray(glam, float)[W] if m else np.zeros(0)
    sol = np.linalg.solve(K, -np.concatenate([g, glw]))
    dx, dl = sol[:n], sol[n:]
    gA = np.zeros((m, n))
    gb = np.zeros(m)
    gA[W] = np.outer(dl, x) + np.outer(lam[W], dx)
    gb[W] = -dl
    gH = 0.5 * (np.outer(dx, x) + np.outer(x, dx))
    return gH, dx.copy(), gA, gb


def certificate(H, A, act, g, glam, gf, gb):
    """kkt_oracle.certificate with the full right-hand side, dx = gf and
    dlam_W = -gb_W:
        |H dx + A_W^T dlam + g|_inf / (1 + |g|_inf + ||H||_inf |dx|_inf)
        |A_W dx + glam_W|_inf / (1 + |glam_W|_inf + ||A||_inf |dx|_inf)"""
    H, A, W, _ = _system(H, A, act)
    g, dx = np.asarray(g, float), np.asarray(gf, float)
    m = A.shape[0]
    dl = -np.asarray(gb, float)[W] if m else np.zeros(0)
    glw = np.asarray(glam, float)[W] if m else np.zeros(0)
    dxn = np.abs(dx).max()
    r1 = H @ dx + A[W].T @ dl + g
    stat = np.abs(r1).max() / (1.0 + np.abs(g).max() + np.abs(H).sum(axis=1).max() * dxn)
    r2 = A[W] @ dx + glw
    An = np.abs(A).sum(axis=1).max() if m else 0.0
    gln = np.abs(glw).max() if len(W) else 0.0
    prim = (np.abs(r2).max() if len(W) else 0.0) / (1.0 + gln + An * dxn)
    return float(stat), float(prim)


def tangent(H, A, act, df, db):
    """One QP: (dx, dlam (m,), 0 outside W) of (x*, lam*) along a change (df, db)
    of (f, b) at fixed active set: H dx + df + A_W^T dlam = 0, A_W dx = db_W."""
    H, A, W, K = _system(H, A, act)
    n, m = H.shape[0], A.shape[0]
    dbw = np.asarray(db, float)[W] if m else np.zeros(0)
    sol = np.linalg.solve(K, np.concatenate([-np.asarray(df, float), dbw]))
    dlam = np.zeros(m)
    dlam[W] = sol[n:]
    return sol[:n].copy(), dlam
