"""TEST INFRASTRUCTURE ONLY: hand-made inputs for qpb_solve_backward, shared by
tests/test_bwd_cases.py (CPU), tests/test_gpu_backward_edges.py and
tests/golden/make_bwd_golden.py (numpy, no GPU).

The backward is a function of the CALLER's active mask, lam and x, so its edges
are reached without a forward solve: every case here is (H, A, mask, x, lam, g)
with a mask of the test's own and a reference that is not the code under test:

    one_hot      QP k has row k alone active: a closed form
    pairs        rows {k, k + 16} (one lane of the n <= 16 kernel) and {31, 32}
                 (the two mask words)
    sizes        |W| in {0, 1, n // 2, n - 1, n} from all m rows, integer data
    overfull     all m bits set, row 5 = row 1 + 2 row 3: more than n bits and
                 a row that is a combination of two earlier ones
    weak         planted.planted_dense's weakly active rows marked active
    conditioned  H = Q diag(logspace(0, -p)) Q^T, cond(H) up to 1e10, with
                 |W| up to n (the references: tests/golden/bwd_cond_*.npz)
    scaled       power-of-two scalings of a `sizes` case, referred to the
                 unscaled reference by the exact scaling law

`rows_in_order` restates in fp64 WHICH rows the kernels count (row order, two
Gram-Schmidt passes, |d2|^2 > 1e-24 |d|^2, at most n); the builders keep every
case far from that threshold on either side, so that the set of rows that count
is never a matter of rounding.  `reference` is tests/kkt_oracle.py on the rows
that count.  `emulate` is the kernels' algebra with one or two projections of
u, for the CPU record of why the second projection exists.
"""
from __future__ import annotations

import os
from typing import NamedTuple

import numpy as np

import kkt_oracle as KO
import planted

NAMES = ("H", "f", "A", "b")
DEP_TOL = 1e-24      # the kernels' kDepTol
KEPT_MIN = 1e-9      # every row that counts has |d2|^2 / |d|^2 at least this
COND_KEPT_MIN = 1e-12  # ... in `conditioned`, where the ratio falls with cond(H): 1.2e-10 at the least
SKIPPED_MAX = 1e-28  # and every skipped one at most this

# the smallest shapes that reach each form of qpb_kkt_bwd.hip, (n, m)
ROUTES = {
    "dense<1,false>": [(7, 14)],
    "dense<2,false>": [(13, 26), (15, 17)],
    "dense<1,true>": [(16, 16), (16, 0)],
    "dense<2,true>": [(16, 32)],
    "wave-n<=16-2words": [(12, 33)],
    "wave-1word": [(20, 0), (20, 7), (24, 32), (17, 1)],
    "wave-2words": [(20, 33), (32, 64)],
}
ALL_ROUTES = [s for v in ROUTES.values() for s in v]
DENSE_ROUTES = [s for k, v in ROUTES.items() if k.startswith("dense") for s in v]
# one shape per kernel form for the cases that need m > n (overfull) or m >= 6
FORM_ROUTES = [(7, 14), (13, 26), (16, 16), (16, 32), (12, 33), (24, 32), (20, 33), (32, 64)]
COND_SHAPES = [(16, 32), (13, 26), (20, 33), (32, 64)]
COND_EXPONENTS = (3, 6, 10)  # cond(H) = 10^p
# (log2 sH, log2 of the rows' factors (alternating in sign), log2 sg); the first is the mildest
# bar (b) of the `conditioned` tests: per array, the error against the 50-digit reference (bwd_harness.rel) is at
# most max(COND_FLOOR, 10 x the numpy oracle's own error on that case).  The floor is 10 x the worst error of the GPU
# kernels on the cond(H) = 1e3 cases against the same reference, MEASURED_1E3: kkt_bwd v1.1 on an MI355X gave 1.77e-14
# at (16, 32), 1.53e-14 at (13, 26), 8.86e-15 at (20, 33) and 1.89e-14 at (32, 64).  The 10 x covers rsq1's one Newton
# step and the order of the sums.
MEASURED_1E3 = 1.89e-14
COND_FLOOR = 10 * MEASURED_1E3
SCALINGS = [(4, 2, -3), (40, 20, 30), (-40, 20, -30), (40, 20, -30), (-40, 20, 30)]


class Case(NamedTuple):
    H: np.ndarray     # (B, n, n)
    A: np.ndarray     # (B, m, n)
    mask: np.ndarray  # (B, m) bool: the caller's active set
    x: np.ndarray     # (B, n)
    lam: np.ndarray   # (B, m)
    g: np.ndarray     # (B, n)
    ref: dict         # NAMES -> the reference gradients
    kept: np.ndarray  # (B, m) bool: the rows of the mask that count (rows_in_order)
    denom: dict = None  # `scaled` only: NAMES -> (B,) the denominators of its pure relative error


def words(mask: np.ndarray) -> np.ndarray:
    """A bool mask (B, m) as qpb.h's active words, int32 (B, ceil(m / 32))."""
    Bq, m = mask.shape
    act = np.zeros((Bq, (m + 31) // 32), np.uint32)
    for i, j in zip(*np.nonzero(mask)):
        act[i, j // 32] |= np.uint32(1) << np.uint32(j % 32)
    return act.view(np.int32)


def sizes_of(n: int, m: int) -> list:
    """|W| in {0, 1, n // 2, n - 1, n}, cut at m, each once."""
    return sorted({min(s, m) for s in (0, 1, n // 2, n - 1, n)})


# ------------------------------------------------------------------ the kernels' algebra in fp64
def _lower_solve(L, B):
    """L X = B by forward substitution (B: (n, k))."""
    X = np.array(B, float)
    for k in range(L.shape[0]):
        X[k] = (X[k] - L[k, :k] @ X[:k]) / L[k, k]
    return X


def _upper_solve(U, B):
    X = np.array(B, float)
    for k in range(U.shape[0] - 1, -1, -1):
        X[k] = (X[k] - U[k, k + 1:] @ X[k + 1:]) / U[k, k]
    return X


def _orthogonalise(H, A, mask):
    """D = A L^{-T}; its rows in the mask, in row order, against the kept rows
    before them in two classical Gram-Schmidt passes.  Returns (L, Q (cnt, n),
    R (cnt, cnt) upper, kept, skipped, ratio (m,), nan outside the mask)."""
    n = H.shape[0]
    m = A.shape[0]
    L = np.linalg.cholesky(H)
    D = _lower_solve(L, A.T).T if m else np.zeros((0, n))
    Q = np.zeros((0, n))
    cols, kept, skipped = [], [], []
    ratio = np.full(m, np.nan)
    for i in np.flatnonzero(mask):
        v = D[i].copy()
        c = np.zeros(len(Q))
        for _ in range(2):
            cc = Q @ v
            c += cc
            v = v - Q.T @ cc
        dd, nd2 = D[i] @ D[i], v @ v
        ratio[i] = nd2 / dd if dd > 0 else 0.0
        if len(Q) < n and nd2 > DEP_TOL * dd:
            cols.append(np.concatenate([c, [np.sqrt(nd2)]]))
            Q = np.concatenate([Q, v[None] / np.sqrt(nd2)])
            kept.append(i)
        else:
            skipped.append(i)
    R = np.zeros((len(kept), len(kept)))
    for t, c in enumerate(cols):
        R[:t + 1, t] = c
    return L, Q, R, np.array(kept, int), np.array(skipped, int), ratio


def rows_in_order(H, A, mask):
    """Which rows of one QP's mask the kernels count: (kept, skipped, ratio),
    ratio[i] = |d2|^2 / |d|^2 of row i (nan outside the mask)."""
    return _orthogonalise(H, A, mask)[3:]


def grads(x, lam, mask, dx, dlam):
    """(gH, gf, gA, gb) of qpb.h from dx and dlam (m, 0 on the rows that do not
    count); lam counts on every row of the mask."""
    lm = np.where(mask, lam, 0.0)
    gH = 0.5 * (np.outer(dx, x) + np.outer(x, dx))
    gA = np.outer(dlam, x) + np.outer(lm, dx)
    return gH, np.array(dx, float), gA, -np.asarray(dlam, float)


def reference(H, A, mask, x, lam, g):
    """One QP: kkt_oracle.backward on the rows that count; a skipped row gets
    gA_i = lam_i dx^T and gb_i = 0 (qpb.h).  Returns (gH, gf, gA, gb)."""
    kept, skipped, _ = rows_in_order(H, A, mask)
    keep = np.zeros(len(mask), bool)
    keep[kept] = True
    gH, gf, gA, gb = KO.backward(H, x, lam, A, keep, g)
    for i in skipped:
        gA[i] = lam[i] * gf
    return gH, gf, gA, gb


def emulate(H, A, mask, g, passes):
    """The kernels' algebra in fp64 with `passes` projections of u = L^{-1} g:
    z = -(u - Q Q^T u), dx = L^{-T} z, R dlam = -Q^T u.  Returns (dx, dlam (m,))."""
    L, Q, R, kept, _, _ = _orthogonalise(H, A, mask)
    z = _lower_solve(L, g[:, None])[:, 0]
    cu = np.zeros(len(Q))
    for _ in range(passes):
        cc = Q @ z
        cu += cc
        z = z - Q.T @ cc
    dx = _upper_solve(L.T, -z[:, None])[:, 0]
    dlam = np.zeros(A.shape[0])
    if len(kept):
        dlam[kept] = _upper_solve(R, -cu[:, None])[:, 0]
    return dx, dlam


# ------------------------------------------------------------------ builders
def _finish(H, A, mask, x, lam, g, ref=None, kept_min=KEPT_MIN) -> Case:
    """Stack, find the rows that count, check the margins, attach the reference."""
    H, A, mask, x, lam, g = (np.ascontiguousarray(v) for v in (H, A, mask, x, lam, g))
    kept = np.zeros(mask.shape, bool)
    for i in range(len(H)):
        k, s, ratio = rows_in_order(H[i], A[i], mask[i])
        kept[i, k] = True
        assert len(k) == 0 or ratio[k].min() >= kept_min, ("kept row near the threshold", i, ratio[k].min())
        assert len(s) == 0 or ratio[s].max() <= SKIPPED_MAX, ("skipped row near the threshold", i, ratio[s].max())
    if ref is None:
        r = [reference(H[i], A[i], mask[i], x[i], lam[i], g[i]) for i in range(len(H))]
        ref = {k: np.array([q[j] for q in r]) for j, k in enumerate(NAMES)}
    return Case(H, A, mask, x, lam, g, ref, kept)


def margins(c: Case):
    """(smallest ratio of a kept row, largest of a skipped row) over the batch; (inf, 0) where there is none."""
    lo, hi = np.inf, 0.0
    for i in range(len(c.H)):
        k, s, ratio = rows_in_order(c.H[i], c.A[i], c.mask[i])
        assert np.array_equal(np.flatnonzero(c.kept[i]), np.sort(k))
        lo = min(lo, ratio[k].min()) if len(k) else lo
        hi = max(hi, ratio[s].max()) if len(s) else hi
    return lo, hi


def _tile(a, count):
    return np.broadcast_to(a, (count,) + a.shape).copy()


def _shared(n, m, seed):
    """One H = I + B^T B / n, m unit-norm rows, x and g: what one_hot and pairs share."""
    rs = np.random.default_rng([seed, n, m])
    B = rs.standard_normal((n, n))
    H = np.eye(n) + B.T @ B / n
    A = rs.standard_normal((m, n))
    A /= np.linalg.norm(A, axis=1, keepdims=True)
    return rs, H, A, rs.standard_normal(n), rs.standard_normal(n)


def one_hot(n: int, m: int) -> Case:
    """m QPs sharing H, A, x, g; QP k has row k alone active with a multiplier
    in [1, 2).  The reference is the closed form, a = a_k:
        dx = -(I - H^{-1} a a^T / (a^T H^{-1} a)) H^{-1} g,  dlam = -a^T H^{-1} g / (a^T H^{-1} a)."""
    rs, H, A, x, g = _shared(n, m, 101)
    lam_k = 1.0 + rs.random(m)
    hg = np.linalg.solve(H, g)
    W = np.linalg.solve(H, A.T)  # H^{-1} a_k in column k
    mask = np.eye(m, dtype=bool)
    lam = np.zeros((m, m))
    ref = []
    for k in range(m):
        a, w = A[k], W[:, k]
        t = (a @ hg) / (a @ w)
        dl = np.zeros(m)
        dl[k] = -t
        lam[k, k] = lam_k[k]
        ref.append(grads(x, lam[k], mask[k], -(hg - w * t), dl))
    ref = {k: np.array([q[j] for q in ref]) for j, k in enumerate(NAMES)}
    return _finish(_tile(H, m), _tile(A, m), mask, _tile(x, m), lam, _tile(g, m), ref)


def pairs(n: int, m: int) -> Case:
    """Masks {k, k + 16} for k < m - 16 (the two rows of one lane of the
    n <= 16 kernel) and {31, 32} where m > 32 (the last bit of the first mask
    word and the first of the second); multipliers of either sign."""
    assert n >= 2 and m > 16
    rs, H, A, x, g = _shared(n, m, 103)
    sets = [(k, k + 16) for k in range(m - 16)] + ([(31, 32)] if m > 32 else [])
    mask = np.zeros((len(sets), m), bool)
    for i, s in enumerate(sets):
        mask[i, list(s)] = True
    lam = np.where(mask, rs.standard_normal(mask.shape), 0.0)
    Q = len(sets)
    return _finish(_tile(H, Q), _tile(A, Q), mask, _tile(x, Q), lam, _tile(g, Q))


def _integer_qp(rs, n, m, size):
    """planted's integer H and rows with `size` rows drawn from all m, redrawn
    until every chosen row counts with a ratio >= KEPT_MIN.  lam is positive
    on the mask and 7 outside it, where the kernels must not read it."""
    while True:
        H = planted._spd(rs, n)
        A = planted._rows(rs, m, n)
        mask = np.zeros(m, bool)
        mask[rs.permutation(m)[:size]] = True
        k, s, ratio = rows_in_order(H, A, mask)
        if len(s) == 0 and (size == 0 or ratio[k].min() >= KEPT_MIN):
            break
    x = rs.integers(-3, 4, n).astype(np.float64)
    lam = np.where(mask, planted._mult(rs, m), 7.0)
    return H, A, mask, x, lam, rs.standard_normal(n)


def sizes(n: int, m: int, reps: int = 2) -> Case:
    """`reps` QPs for each |W| of sizes_of(n, m), interleaved so that the QPs
    of a wavefront differ in size."""
    rs = np.random.default_rng([107, n, m])
    qs = [_integer_qp(rs, n, m, s) for _ in range(reps) for s in sizes_of(n, m)]
    return _finish(*(np.stack(v) for v in zip(*qs)))


def _overfull_qp(rs, n, m):
    assert m >= 6 and n >= 3
    for _ in range(100):
        H = planted._spd(rs, n)
        A = planted._rows(rs, m, n)
        A[5] = A[1] + 2.0 * A[3]
        mask = np.ones(m, bool)
        k, s, ratio = rows_in_order(H, A, mask)
        if 5 in s and ratio[k].min() >= KEPT_MIN and ratio[s].max() <= SKIPPED_MAX:
            break
    x = rs.integers(-3, 4, n).astype(np.float64)
    return H, A, mask, x, planted._mult(rs, m), rs.standard_normal(n)


def overfull(n: int, m: int, count: int = 5) -> Case:
    """ALL m bits set, integer rows, row 5 = row 1 + 2 row 3: row 5 is skipped
    as a combination of two earlier rows, and with m > n the rows met after n
    have counted are skipped as well.  Every row has a positive multiplier."""
    rs = np.random.default_rng([109, n, m])
    return _finish(*(np.stack(v) for v in zip(*[_overfull_qp(rs, n, m) for _ in range(count)])))


def weak(n: int, m: int, count: int = 6) -> Case:
    """planted_dense(..., "weak"): all its tight rows marked active, lam = 0 on
    the weakly active half of them (and 7 outside the mask)."""
    qs = []
    for i in range(count):
        p = planted.planted_dense(n, m, planted.seed_of(n, m) + i, "weak")
        assert (p.lam[p.tight] == 0).any() and (p.lam[p.tight] > 0).any()
        g = np.random.default_rng([113, n, m, i]).standard_normal(n)
        qs.append((p.H, p.A, p.tight, p.x, np.where(p.tight, p.lam, 7.0), g))
    return _finish(*(np.stack(v) for v in zip(*qs)))


def conditioned_inputs(n: int, m: int):
    """The ill-conditioned family, one QP per (p, |W|) of COND_EXPONENTS x
    sizes_of(n, m): H = Q diag(logspace(0, -p, n)) Q^T with Q from the QR of a
    Gaussian matrix, rows of A with N(0, 1) entries, |W| rows drawn from all
    m, g ~ N(0, I), x ~ N(0, I), lam in [1, 2) on the mask.
    Returns (H, A, mask, x, lam, g, p (B,), size (B,))."""
    rs = np.random.default_rng([127, n, m])
    out = []
    for p in COND_EXPONENTS:
        for s in sizes_of(n, m):
            Q = np.linalg.qr(rs.standard_normal((n, n)))[0]
            H = (Q * np.logspace(0, -p, n)) @ Q.T
            H = 0.5 * (H + H.T)
            A = rs.standard_normal((m, n))
            mask = np.zeros(m, bool)
            mask[rs.permutation(m)[:s]] = True
            lam = np.where(mask, 1.0 + rs.random(m), 0.0)
            out.append((H, A, mask, rs.standard_normal(n), lam, rs.standard_normal(n), p, s))
    return tuple(np.stack(v) for v in zip(*out))


def conditioned(n: int, m: int) -> Case:
    """conditioned_inputs with the numpy oracle as `ref` (the 40-digit
    references are the fixture's: tests/golden/bwd_cond_n{n}_m{m}.npz)."""
    return _finish(*conditioned_inputs(n, m)[:6], kept_min=COND_KEPT_MIN)


def conditioned_fixture(n: int, m: int):
    """The committed `conditioned` cases of one shape with their 50-digit
    references (tests/golden/make_bwd_golden.py): (Case, p (B,), size (B,),
    oracle_err (B, 4): the numpy oracle's own error per array of NAMES)."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"bwd_cond_n{n}_m{m}.npz"))
    ref = [grads(z["x"][i], z["lam"][i], z["mask"][i], z["dx"][i], z["dlam"][i]) for i in range(len(z["H"]))]
    ref = {k: np.array([q[j] for q in ref]) for j, k in enumerate(NAMES)}
    c = Case(z["H"], z["A"], z["mask"], z["x"], z["lam"], z["g"], ref, z["mask"].copy())
    return c, z["p"], z["size"], z["oracle_err"]


def scaled(c: Case, eH: int, eA: int, eg: int) -> Case:
    """H 2^eH, row i of A times a_i = 2^(+eA) (i even) or 2^(-eA) (i odd),
    g 2^eg; x and lam as they are.  Powers of two commute with every rounding,
    so the reference is the unscaled one under the exact scaling law
        dx' = (sg / sH) dx,  dlam'_i = sg dlam_i / a_i
    with gH, gA, gb formed from those: no second solve.

    The error measure of a scaled case is purely relative, max|delta| /
    `denom`, denom = max|ref| per QP and array.  Where n rows count, dx is 0
    in exact arithmetic (the oracle holds rounding noise there): the reference
    dx is set to exactly 0 and gf and gH are measured against the same QP's
    unconstrained step -(sg / sH) H^{-1} g, the scale any rounding error of
    dx lives on."""
    n, m = c.H.shape[1], c.A.shape[1]
    sH, sg = 2.0 ** eH, 2.0 ** eg
    a = 2.0 ** np.where(np.arange(m) % 2 == 0, eA, -eA).astype(float)
    ref, denom = [], []
    for i in range(len(c.H)):
        full = c.kept[i].sum() == n
        dx = np.zeros(n) if full else c.ref["f"][i] * (sg / sH)
        dl = -c.ref["b"][i] * sg / a
        assert (dl[c.mask[i] & ~c.kept[i]] == 0.0).all()
        r = grads(c.x[i], c.lam[i], c.mask[i], dx, dl)
        d = [np.abs(v).max() if v.size else 0.0 for v in r]
        if full:
            free = grads(c.x[i], c.lam[i], c.mask[i], -np.linalg.solve(c.H[i], c.g[i]) * (sg / sH), np.zeros(m))
            d[0], d[1] = np.abs(free[0]).max(), np.abs(free[1]).max()
        ref.append(r)
        denom.append(d)
    ref = {k: np.array([q[j] for q in ref]) for j, k in enumerate(NAMES)}
    denom = {k: np.array([q[j] for q in denom]) for j, k in enumerate(NAMES)}
    return Case(c.H * sH, c.A * a[None, :, None], c.mask, c.x, c.lam, c.g * sg, ref, c.kept, denom)


def pure(a, c: Case, k: str):
    """The pure relative error of array k of a scaled case per QP; where the
    denominator is 0 (no row counts: gA and gb are all zero) only 0 passes."""
    d = np.abs(a - c.ref[k]).reshape(len(a), -1).max(axis=1) if a[0].size else np.zeros(len(a))
    r = c.denom[k]
    return np.where(r > 0, d / np.where(r > 0, r, 1.0), np.where(d > 0, np.inf, 0.0))
