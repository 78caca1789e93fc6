"""TEST INFRASTRUCTURE ONLY: the oracle for qpb_solve_box_backward (numpy, no GPU).

For a box lb <= x <= ub the KKT system of tests/kkt_oracle.py at a fixed active
set collapses.  Variable j is FIXED when its upper-bound bit (j) or its
lower-bound bit (n + j) is set in the mask; F are the free variables:

    dx_fixed = 0            H_FF dx_F = -g_F
    r = g + H dx            (zero on F by construction)
    gf = dx                 gH = 1/2 (dx x^T + x dx^T)
    gub_j = r_j  if the upper bound of j is active, else 0
    glb_j = r_j  if the lower bound of j is active and the upper is not, else 0

`backward` is these formulas.  `dense_form` restates a box case for
kkt_oracle.backward / kkt_oracle.certificate on the explicit A = [I; -I]
(gub = gb[:n], glb = -gb[n:]), the reference the formulas and the kernels are
held against.  `family` is tests/test_gpu_box.py's `_family` (asymmetric
bounds around 0), `cycled` a batch whose QPs cycle through WIDTHS so that the
neighbours in a wavefront have different masks, and `solve` the CPU forward
(oracle.active_set_solve on the dense form).
"""
from __future__ import annotations

import numpy as np

import oracle as O

NAMES = ("H", "f", "lb", "ub")
WIDTHS = (10.0, 1.0, 0.1)


def family(seed: int, count: int, n: int, width: float):
    """The conditioned family's H and f with bounds lb < 0 < ub:
    lb ~ -U(0.5, 1.5) width, ub ~ U(0.5, 1.5) width.  Returns (H, f, lb, ub)."""
    H, f, _, _ = O.family_conditioned(seed, count, n, m=2 * n, box=width, kind="box")
    rs = np.random.default_rng(seed + 1)
    ub = rs.uniform(0.5, 1.5, size=(count, n)) * width
    lb = -rs.uniform(0.5, 1.5, size=(count, n)) * width
    return H, f, lb, ub


def cycled(seed: int, count: int, n: int):
    """`family` with QP i at width WIDTHS[i % 3].  Returns (H, f, lb, ub, width (count,))."""
    parts = [family(seed, count, n, w) for w in WIDTHS]
    pick = np.arange(count) % len(WIDTHS)
    out = [np.ascontiguousarray(np.stack([parts[pick[i]][k][i] for i in range(count)])) for k in range(4)]
    return (*out, np.array(WIDTHS)[pick])


def dense(lb, ub):
    """The explicit rows of a batch of boxes: A = [I; -I] (B, 2n, n), b = [ub; -lb]."""
    B, n = lb.shape
    A = np.concatenate([np.broadcast_to(np.eye(n), (B, n, n)), np.broadcast_to(-np.eye(n), (B, n, n))], axis=1)
    return np.ascontiguousarray(A), np.concatenate([ub, -lb], axis=1)


def solve(H, f, lb, ub):
    """The batch on the CPU: (x (B, n), lam (B, 2n), mask (B, 2n) bool), every QP solved."""
    A, b = dense(lb, ub)
    res = [O.active_set_solve(H[i], f[i], A[i], b[i]) for i in range(len(H))]
    assert all(r.status == 0 for r in res)
    return np.array([r.x for r in res]), np.array([r.lam for r in res]), np.array([r.active for r in res])


def backward(H, x, mask, g):
    """One QP by the reduced formulas: (gH, gf, glb, gub).  mask: bool (2n,),
    upper bounds first."""
    H, x, g = (np.asarray(v, float) for v in (H, x, g))
    n = H.shape[0]
    up, lo = np.asarray(mask[:n], bool), np.asarray(mask[n:], bool)
    free = np.flatnonzero(~(up | lo))
    dx = np.zeros(n)
    if len(free):
        dx[free] = np.linalg.solve(H[np.ix_(free, free)], -g[free])
    r = g + H @ dx
    gH = 0.5 * (np.outer(dx, x) + np.outer(x, dx))
    return gH, dx, np.where(lo & ~up, r, 0.0), np.where(up, r, 0.0)


def backward_batch(H, x, mask, g):
    """`backward` over a batch: a dict over NAMES."""
    out = [backward(H[i], x[i], mask[i], g[i]) for i in range(len(H))]
    return {k: np.array([o[j] for o in out]) for j, k in enumerate(NAMES)}


def dense_mask(mask):
    """The box mask (.., 2n) as the mask of linearly independent rows of
    A = [I; -I]: the lower bit dropped where both bits of a variable are set
    (the upper bound comes first in row order)."""
    mask = np.asarray(mask, bool)
    n = mask.shape[-1] // 2
    out = mask.copy()
    out[..., n:] &= ~mask[..., :n]
    return out


def to_gb(gub, glb):
    """(gub, glb) as kkt_oracle's gb over the rows of A = [I; -I], b = [ub; -lb]."""
    return np.concatenate([gub, -np.asarray(glb)], axis=-1)


def dense_form(H, x, mask, g):
    """kkt_oracle.backward on the explicit A = [I; -I] (lam plays no part in
    gH, gf and gb), as a dict over NAMES.  H, x, g batched, mask (B, 2n)."""
    import kkt_oracle as KO
    Bq, n = g.shape
    A = dense(np.zeros((1, n)), np.zeros((1, n)))[0][0]
    dm = dense_mask(mask)
    out = {k: [] for k in NAMES}
    for i in range(Bq):
        gH, gf, _, gb = KO.backward(H[i], x[i], np.zeros(2 * n), A, dm[i], g[i])
        out["H"].append(gH)
        out["f"].append(gf)
        out["ub"].append(gb[:n])
        out["lb"].append(-gb[n:])
    return {k: np.array(v) for k, v in out.items()}


def certificates(H, mask, g, out):
    """kkt_oracle.certificate of a batch of box outputs on the explicit A:
    (B, 2) = (stat, prim) per QP."""
    import kkt_oracle as KO
    Bq, n = g.shape
    A = dense(np.zeros((1, n)), np.zeros((1, n)))[0][0]
    dm = dense_mask(mask)
    gb = to_gb(out["ub"], out["lb"])
    return np.array([KO.certificate(H[i], A, dm[i], g[i], out["f"][i], gb[i]) for i in range(Bq)])
