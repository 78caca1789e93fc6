"""TEST INFRASTRUCTURE ONLY: the oracle for qpb_solve_box_backward_dual (numpy, no GPU).

The KKT system of tests/dual_oracle.py on A = [I; -I] at a fixed active set,
with the unit rows eliminated.  S are the fixed variables, F the free ones, and
glam (2n,) is in qpb_solve_box's lam layout, the upper bounds' entries first:

    d_j = -glam[j]        the upper bit of j is set
    d_j = +glam[n + j]    only the lower bit of j is set
    d_j = 0               j is free
    dx_S = d_S            H_FF dx_F = -g_F - H_FS d_S
    r = g + H dx
    gf = dx               gH = 1/2 (dx x^T + x dx^T)
    gub_j = r_j  if the upper bound of j is active, else 0
    glb_j = r_j  if the lower bound of j is active and the upper is not, else 0

`backward` is these formulas; `tangent` reads them as the forward sensitivity of
(x*, lam*) along (df, dlb, dub); `prescribed` is d alone.  The entries of glam
at a clear bit, and at the lower bit of a variable whose both bits are set, are
never read.
"""
from __future__ import annotations

import numpy as np

from box_bwd_oracle import NAMES


def prescribed(mask, glam):
    """d (n,) of one QP: mask bool (2n,), upper bounds first."""
    mask = np.asarray(mask, bool)
    n = mask.shape[0] // 2
    up, lo = mask[:n], mask[n:]
    d = np.zeros(n)
    for j in range(n):
        if up[j]:
            d[j] = -glam[j]
        elif lo[j]:
            d[j] = glam[n + j]
    return d


def backward(H, x, mask, g, glam):
    """One QP by the closed form: (gH, gf, glb, gub)."""
    H, x, g = (np.asarray(v, float) for v in (H, x, g))
    n = H.shape[0]
    up, lo = np.asarray(mask[:n], bool), np.asarray(mask[n:], bool)
    fixed = up | lo
    free, fix = np.flatnonzero(~fixed), np.flatnonzero(fixed)
    dx = prescribed(mask, glam)
    if len(free):
        dx[free] = np.linalg.solve(H[np.ix_(free, free)], -g[free] - H[np.ix_(free, fix)] @ dx[fix])
    r = g + H @ dx
    gH = 0.5 * (np.outer(dx, x) + np.outer(x, dx))
    return gH, dx, np.where(lo & ~up, r, 0.0), np.where(up, r, 0.0)


def backward_batch(H, x, mask, g, glam):
    """`backward` over a batch: a dict over box_bwd_oracle.NAMES."""
    out = [backward(H[i], x[i], mask[i], g[i], glam[i]) for i in range(len(H))]
    return {k: np.array([o[j] for o in out]) for j, k in enumerate(NAMES)}


def tangent(H, mask, df, dlb=None, dub=None):
    """One QP: (dx, dlam (2n,)) of (x*, lam*) along a change (df, dlb, dub) of
    (f, lb, ub) at fixed active set: gx = df, glam = [-dub, +dlb], and
    dx = gf, dlam = [-gub, +glb]."""
    n = np.asarray(H).shape[0]
    dlb = np.zeros(n) if dlb is None else np.asarray(dlb, float)
    dub = np.zeros(n) if dub is None else np.asarray(dub, float)
    _, dx, glb, gub = backward(H, np.zeros(n), mask, df, np.concatenate([-dub, dlb]))
    return dx, np.concatenate([-gub, glb])
