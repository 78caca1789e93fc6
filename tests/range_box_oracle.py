"""TEST INFRASTRUCTURE ONLY: inputs and the oracle for qpb_solve_range_box (numpy, no GPU).

    min 1/2 x^T H x + f^T x   s.t.   G[:meq] x = bu[:meq],  bl <= G x <= bu,  lb <= x <= ub

The specification of the call is qpb_solve_range on the materialised problem
A' = [G; I], bl' = [bl; lb], bu' = [bu; ub], so the oracle is range_oracle's on
exactly that: materialise() builds it, box_reference() solves it once per shape.

The family is range_oracle.range_family's rows (strictly feasible at xc, slack
>= 1 on both sides) with a box around xc that is tight enough to bind: half the
mean distance from xc to the unconstrained minimiser, times U(0.1, 1) per
variable and side.
"""
from __future__ import annotations

import numpy as np

import range_oracle as RO

# (n, mg, meq): the three load paths of gi_dense at one and two rows per lane,
# rows straddling the lane-row boundary, mg = 0, meq > 0, the class edge
# (16, 17) and the padded and full wave forms
DENSE_SHAPES = [(16, 16, 0), (16, 16, 2), (16, 7, 0), (16, 1, 1), (16, 0, 0),
                (12, 20, 0), (3, 29, 0), (5, 3, 1), (7, 9, 2), (2, 1, 1), (1, 1, 0)]
WAVE_SHAPES = [(16, 17, 1), (17, 20, 0), (20, 9, 0), (32, 32, 3), (32, 5, 0), (32, 0, 0)]
SHAPES = DENSE_SHAPES + WAVE_SHAPES


def box_family(count: int, n: int, mg: int, meq: int):
    """(H, f, G, bl, bu, lb, ub, xc): G, bl, bu are (count, mg, n) and (count, mg),
    with mg = 0 allowed."""
    H, f, G, bl, bu, xc = RO.range_family(count, n, max(mg, 1), meq)
    if mg == 0:  # the one row is dropped
        G, bl, bu = G[:, :0], bl[:, :0], bu[:, :0]
    rng = np.random.default_rng([RO.SEED_BASE + n + meq, 0xB0C5])
    x0 = -np.linalg.solve(H, f[:, :, None])[:, :, 0]
    d = np.abs(x0 - xc).mean(axis=1, keepdims=True)
    ub = xc + rng.uniform(0.1, 1.0, size=xc.shape) * 0.5 * d
    lb = xc - rng.uniform(0.1, 1.0, size=xc.shape) * 0.5 * d
    return H, f, G, bl, bu, lb, ub, xc


def materialise(G, bl, bu, lb, ub, n: int):
    """([G; I], [bl; lb], [bu; ub]) of a batch; a None half is -inf / +inf."""
    B = len(lb if lb is not None else ub if ub is not None else bl if bl is not None else bu)
    mg = 0 if G is None else G.shape[-2]
    Gb = np.zeros((B, 0, n)) if G is None else np.broadcast_to(G, (B, mg, n))
    A = np.concatenate([Gb, np.broadcast_to(np.eye(n), (B, n, n))], axis=1)
    half = lambda v, k, fill: np.full((B, k), fill) if v is None else np.asarray(v, float)  # noqa: E731
    lo = np.concatenate([half(bl, mg, -np.inf), half(lb, n, -np.inf)], axis=1)
    hi = np.concatenate([half(bu, mg, np.inf), half(ub, n, np.inf)], axis=1)
    return np.ascontiguousarray(A), lo, hi


_CACHE = {}


def box_reference(count: int, n: int, mg: int, meq: int):
    """(family, (A', bl', bu'), refs): the family, its materialised problem and
    range_oracle.range_solve on it, solved once per session and shared (never
    modified) by the tests that need it."""
    key = (count, n, mg, meq)
    if key not in _CACHE:
        fam = box_family(count, n, mg, meq)
        H, f, G, bl, bu, lb, ub, xc = fam
        A, lo, hi = materialise(G, bl, bu, lb, ub, n)
        refs = [RO.range_solve(H[i], f[i], A[i], lo[i], hi[i], meq, xc[i]) for i in range(count)]
        _CACHE[key] = (fam, (A, lo, hi), refs)
    return _CACHE[key]
