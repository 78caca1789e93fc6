"""TEST INFRASTRUCTURE ONLY: the oracle for qpb_solve_range (numpy, no GPU).

    min 1/2 x^T H x + f^T x   s.t.   E x = d,  hl <= G x <= hu
    with A = [E; G], bu = [d; hu], bl = [.; hl], E = A[:meq]  (qpb.h's row order)

The kernels take a two-sided row natively; the oracle does not.  It maps the
problem to the pair form

    A' = [E; G; -G],  b' = [d; hu; -hl],  meq equalities

solves that with eq_oracle.eq_solve and maps the result back:
lam = lam_up - lam_lo, active = up | lo, lower = lo (rows < meq: lam as it is,
active, never lower).  A side whose bound is not finite gets b' = +inf there (a
row that is never active).
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

import eq_oracle as EO

SEED_BASE = 11  # range_family's seed is SEED_BASE + n + meq


def range_family(count: int, n: int, m: int, meq: int):
    """eq_oracle.eq_family(11 + n + meq, ...) with bu = b and
    bl = A xc - U(0.1, 1) 10 (bl[:, :meq] = bu[:, :meq]): xc stays strictly
    feasible, slack >= 1 on both sides.  Returns (H, f, A, bl, bu, xc)."""
    seed = SEED_BASE + n + meq
    H, f, A, bu, xc = EO.eq_family(seed, count, n, m, meq)
    rng = np.random.default_rng([seed, 0x7A9E])
    bl = np.einsum("bij,bj->bi", A, xc) - rng.uniform(0.1, 1.0, size=bu.shape) * 10.0
    bl[:, :meq] = bu[:, :meq]
    return H, f, A, bl, bu, xc


def to_pairs(A, bl, bu, meq: int):
    """One QP or a batch (leading axes kept): ([E; G; -G], [d; hu; -hl]) with
    non-finite bounds as +inf."""
    A, bl, bu = (np.asarray(v, float) for v in (A, bl, bu))
    G = A[..., meq:, :]
    hu = np.where(np.isfinite(bu[..., meq:]), bu[..., meq:], np.inf)
    hl = np.where(np.isfinite(bl[..., meq:]), bl[..., meq:], -np.inf)
    return (np.concatenate([A[..., :meq, :], G, -G], axis=-2),
            np.concatenate([bu[..., :meq], hu, -hl], axis=-1))


class RangeResult(NamedTuple):
    x: np.ndarray
    lam: np.ndarray     # (m,) signed
    active: np.ndarray  # (m,) bool, either side
    lower: np.ndarray   # (m,) bool, active at bl
    iters: int
    status: int


def from_pairs(lam2, act2, m: int, meq: int):
    """(lam, active, lower) of the m range rows from the pair form's 2m - meq."""
    k = m - meq
    lam2, act2 = np.asarray(lam2, float), np.asarray(act2, bool)
    lam = np.concatenate([lam2[:meq], lam2[meq:meq + k] - lam2[meq + k:]])
    up, lo = act2[meq:meq + k], act2[meq + k:]
    active = np.concatenate([act2[:meq], up | lo])
    lower = np.concatenate([np.zeros(meq, bool), lo])
    return lam, active, lower


def range_solve(H, f, A, bl, bu, meq: int, xc) -> RangeResult:
    """One QP through the pair form and eq_oracle.eq_solve.  The rows of the pair
    form whose bound is +inf (an absent side) are left out of the solve: they
    are never active, and the primal active-set oracle is not made for them."""
    A2, b2 = to_pairs(A, bl, bu, meq)
    keep = np.isfinite(b2)
    keep[:meq] = True
    r = EO.eq_solve(H, f, A2[keep], b2[keep], meq, xc)
    lam2, act2 = np.zeros(len(b2)), np.zeros(len(b2), bool)
    lam2[keep], act2[keep] = r.lam, r.active
    lam, active, lower = from_pairs(lam2, act2, np.asarray(A).shape[0], meq)
    return RangeResult(r.x, lam, active, lower, r.iters, r.status)


def kkt_range(H, f, A, bl, bu, meq: int, x, lam):
    """The certificate of a batch of range solutions, relative residuals on
    oracle.kkt_residuals' scales: stationarity with the signed lam; feasibility
    on both sides (and |E x - d|) in `prim`; `dual`: a row strictly below bu
    (by more than 1e-9 of the scale) must have lam <= 0 and a row strictly
    above bl lam >= 0, the wrong-signed part is the residual; `comp`: |lam|
    times the slack of the side its sign names.  Rows < meq are free in sign."""
    H, f, A, bl, bu, x, lam = (np.asarray(v, float) for v in (H, f, A, bl, bu, x, lam))
    m = A.shape[1]
    r = np.einsum("bij,bj->bi", H, x) + f + np.einsum("bij,bi->bj", A, lam)
    xn = np.abs(x).max(axis=1)
    Hn = np.abs(H).sum(axis=2).max(axis=1)
    stat = np.abs(r).max(axis=1) / (1.0 + np.abs(f).max(axis=1) + Hn * xn)
    An = np.abs(A).sum(axis=2).max(axis=1)
    fin = lambda v: np.where(np.isfinite(v), np.abs(v), 0.0)  # noqa: E731
    sc = 1.0 + np.maximum(fin(bu).max(axis=1), fin(bl[:, meq:]).max(axis=1, initial=0.0)) + An * xn
    ax = np.einsum("bij,bj->bi", A, x)
    hu = np.where(np.isfinite(bu), bu, np.inf)
    hl = np.where(np.isfinite(bl), bl, -np.inf)
    su, sl = hu - ax, ax - hl  # slacks of the two sides, >= 0 when feasible
    z = np.zeros(len(x))
    res = np.abs(su[:, :meq]).max(axis=1) if meq else z
    ln = 1.0 + np.abs(lam).max(axis=1)
    if meq < m:
        viol = np.maximum(0.0, -np.minimum(su[:, meq:], sl[:, meq:]).min(axis=1))
        li = lam[:, meq:]
        # a positive multiplier names the upper side, a negative one the lower
        side = np.where(li > 0, su[:, meq:], np.where(li < 0, sl[:, meq:], 0.0))
        with np.errstate(invalid="ignore"):
            comp = np.abs(li * side)
        comp = np.where(li == 0, 0.0, comp).max(axis=1) / (ln * sc)
        # lam >= 0 where a x > bl strictly, lam <= 0 where a x < bu strictly: with
        # both slacks positive beyond the scale's rounding the multiplier is 0
        tol = 1e-9 * sc[:, None]
        wrong = np.where((li > 0) & (su[:, meq:] > tol), li, 0.0) + np.where((li < 0) & (sl[:, meq:] > tol), -li, 0.0)
        dual = wrong.max(axis=1) / ln
    else:
        viol, comp, dual = z, z, z
    prim = np.maximum(viol, res) / sc
    return {"stat": stat, "prim": prim, "dual": dual, "comp": comp}


def pack_bits(mask):
    """(B, m) bool -> (B, ceil(m/32)) uint32, bit i of word i // 32 for row i."""
    mask = np.asarray(mask, bool)
    B, m = mask.shape
    w = (m + 31) // 32
    pad = np.zeros((B, 32 * w), bool)
    pad[:, :m] = mask
    weights = (1 << np.arange(32, dtype=np.uint64))
    return (pad.reshape(B, w, 32) * weights).sum(axis=2).astype(np.uint32)


def unpack_bits(words, m: int):
    """(B, ceil(m/32)) 32-bit words (any integer dtype) -> (B, m) bool."""
    words = np.asarray(words).astype(np.int64) & 0xFFFFFFFF
    rows = np.arange(m)
    return ((words[:, rows // 32] >> (rows % 32)) & 1).astype(bool)


_CACHE = {}


def range_reference(count: int, n: int, m: int, meq: int):
    """(H, f, A, bl, bu, xc, refs) of range_family, solved once per session and
    shared (never modified) by the tests that need it."""
    key = (count, n, m, meq)
    if key not in _CACHE:
        H, f, A, bl, bu, xc = range_family(count, n, m, meq)
        refs = [range_solve(H[i], f[i], A[i], bl[i], bu[i], meq, xc[i]) for i in range(count)]
        assert all(r.status == 0 for r in refs), key
        _CACHE[key] = (H, f, A, bl, bu, xc, refs)
    return _CACHE[key]


def side_counts(count: int, n: int, m: int, meq: int):
    """(upper, lower, opposite) over a reference batch: active rows >= meq on each
    side, and those active on the side opposite to the one violated at the
    unconstrained minimum x0 = -H^-1 f (the rows that reach a kernel's
    re-orientation)."""
    H, f, A, bl, bu, _, refs = range_reference(count, n, m, meq)
    up = lo = opp = 0
    for i, r in enumerate(refs):
        a0 = A[i] @ -np.linalg.solve(H[i], f[i])
        for j in range(meq, m):
            if not r.active[j]:
                continue
            lo += bool(r.lower[j])
            up += not r.lower[j]
            if r.lower[j]:
                opp += bool(a0[j] > bu[i, j])
            else:
                opp += bool(a0[j] < bl[i, j])
    return up, lo, opp
