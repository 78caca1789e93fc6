"""TEST INFRASTRUCTURE ONLY: QPs with a planted, exact solution (numpy, no GPU).

The oracle (oracle/oracle.py) is a primal active-set method and can run into
its iteration cap at a degenerate vertex (tests/test_planted.py pins what it
still gets right there), so the degenerate families need a reference that is
not a solver.  Here the solution comes first and the QP is built around it:

    pick x*, lam* >= 0 and the tight rows, then
    b = A x* + slack (slack = 0 on the tight rows),  f = -H x* - A^T lam*

All data are small integers held in fp64, so b, f and every tight row are
exact and the KKT residuals of (x*, lam*) are exactly 0.0.  H is SPD, so x* is
THE solution; lam* is one valid multiplier and the only one when the tight
rows are linearly independent.

    planted_dense  weak / dup / vertex / ties     A x <= b
    planted_eq     weak / dup on the rows >= meq  rows < meq are equalities
    planted_box    weak / pinned / all_pinned / ties   lb <= x <= ub
    one_hot_rows, one_hot_bounds, one_hot_eq
                   m QPs sharing H, f, A in which QP k violates row k alone
                   (closed form), so that every row index is the active one once

Routes (the smallest shapes that reach each kernel form) are restated from
tests/test_gpu_status_contract.py so that the CPU test of this module and the
GPU tests use the same shapes and seeds.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

FLAG_MIXED, FLAG_DIAG_WAVE = 32, 256

# (kernel form, n, m, batch, qpb_desc.flags): test_gpu_status_contract.DENSE and the Gram kernel's full tile set
DENSE = [
    ("gi_dense-mr1-padded", 7, 14, 37, 0),
    ("gi_dense-mr2-padded", 13, 26, 37, 0),
    ("gi_dense-n16-mr1", 16, 16, 37, 0),
    ("gi_dense-full", 16, 32, 37, 0),
    ("gi_wave-diag", 7, 14, 13, FLAG_DIAG_WAVE),
    ("gi_wave-20x33", 20, 33, 13, 0),
    ("gi_wave-32x64", 32, 64, 13, 0),
    ("gi_mixed", 20, 33, 13, FLAG_MIXED),
    ("gi_gram-33x40", 33, 40, 6, 0),
    ("gi_gram-48x96", 48, 96, 6, 0),
]
GRAM_FULL = ("gi_gram-128x256", 128, 256, 2, 0)
DEGENERATE = DENSE + [GRAM_FULL]
# (n, m, meq, batch): the EQ forms of gi_dense and gi_wave
EQ = [(16, 32, 4, 37), (20, 33, 5, 13)]
# (n, batch): gi_box padded and full, gi_wave's BOX form, gi_gram's, and its full tile set
BOX = [(7, 13), (16, 13), (20, 13), (40, 13), (128, 2)]
# one-hot shapes: every dense route, a one-word-per-tile-crossing m = 65 at small n, the full Gram tile set
ONE_HOT = DENSE + [("gi_gram-12x65", 12, 65, 65, 0), GRAM_FULL]
ONE_HOT_BOX_N = [7, 16, 20, 32, 40, 128]

DENSE_KINDS = ("weak", "dup", "vertex")
EQ_KINDS = ("weak", "dup")
BOX_KINDS = ("weak", "pinned", "all_pinned")
_KIND_ID = {"weak": 1, "dup": 2, "vertex": 3, "pinned": 4, "all_pinned": 5}


def seed_of(n: int, m: int) -> int:
    """The seed every planted and one-hot family uses at a shape."""
    return 31 * n + m


class Planted(NamedTuple):
    H: np.ndarray
    f: np.ndarray
    A: np.ndarray
    b: np.ndarray
    x: np.ndarray      # x*
    lam: np.ndarray    # lam* (one valid multiplier)
    tight: np.ndarray  # bool: a_i x* == b_i
    group: np.ndarray  # int: the `dup` triple a row belongs to, -1 outside the triples


class PlantedBox(NamedTuple):
    H: np.ndarray
    f: np.ndarray
    lb: np.ndarray
    ub: np.ndarray
    x: np.ndarray
    lam: np.ndarray      # 2n: upper bounds' multipliers, then the lower bounds' (qpb.h's order)
    tight: np.ndarray    # 2n bool, the same order
    mu: np.ndarray       # n: lam_ub - lam_lb, the unique signed multiplier of variable j
    pinned: np.ndarray   # n bool: lb_j == ub_j
    plain: np.ndarray    # n bool: neither pinned nor weakly active (the bits of j are determined)
    A: np.ndarray        # [I; -I]
    b: np.ndarray        # [ub; -lb]


def _spd(rs, n):
    """H = B^T B + n I, B integer in [-2, 2]: cond(H) about 4-9."""
    B = rs.integers(-2, 3, (n, n)).astype(np.float64)
    return B.T @ B + n * np.eye(n)


def _rows(rs, k, n):
    """k integer rows in [-3, 3]; an all-zero row gets a 1 in column 0."""
    A = rs.integers(-3, 4, (k, n)).astype(np.float64)
    A[~A.any(axis=1), 0] = 1.0
    return A


def _independent_rows(rs, k, n, first=None):
    """_rows, redrawn until [first; rows] has full row rank (needs rows <= n)."""
    base = np.zeros((0, n)) if first is None else first
    assert len(base) + k <= n, (len(base), k, n)
    while True:
        A = _rows(rs, k, n)
        if np.linalg.matrix_rank(np.concatenate([base, A])) == len(base) + k:
            return A


def _mult(rs, k):
    return rs.integers(1, 5, k).astype(np.float64)


def _plant_rows(rs, n, m, kind, first=None):
    """The inequality rows of one QP before the permutation: (A, lam, tight,
    group) with the tight rows first.  `first`: equality rows the independent
    tight rows must also be independent of (planted_eq)."""
    n_free = n - (0 if first is None else len(first))
    A = _rows(rs, m, n)
    lam = np.zeros(m)
    tight = np.zeros(m, bool)
    group = -np.ones(m, np.int64)
    if kind == "weak":
        k = max(1, min(n_free // 3, m // 3))
        A[:2 * k] = _independent_rows(rs, 2 * k, n, first)
        lam[:k] = _mult(rs, k)
        tight[:2 * k] = True
    elif kind == "dup":
        k = max(1, min(n_free // 2, m // 3))
        A[:k] = _independent_rows(rs, k, n, first)
        A[k:2 * k] = A[:k]
        A[2 * k:3 * k] = 2.0 * A[:k]
        lam[:k] = _mult(rs, k)
        tight[:3 * k] = True
        group[:3 * k] = np.tile(np.arange(k), 3)
    elif kind == "vertex":
        t = min(m, n + max(1, n // 2))
        lam[:max(1, n // 2)] = _mult(rs, max(1, n // 2))
        tight[:t] = True
    else:
        raise ValueError(kind)
    return A, lam, tight, group


def _ties_dense(n, m):
    """H = I, f = -3, rows e_0 .. e_{n-1}, then -e_0 .. -e_{n-1}, all with
    b = 1, cut at m rows; rows past 2n are -e_j with b = 2 + (i - 2n) (never
    tight).  The unconstrained minimiser 3 * 1 violates every upper row by the
    same 2 with the same row norm: exact ties in the selection key.  x* = 1 on
    the bounded variables (3 elsewhere), lam* = 2 on the upper rows: strictly
    complementary and independent, so the active set is unique."""
    A = np.zeros((m, n))
    b = np.ones(m)
    for i in range(m):
        if i < n:
            A[i, i] = 1.0
        else:
            A[i, (i - n) % n] = -1.0
            if i >= 2 * n:
                b[i] = 2.0 + (i - 2 * n)
    up = np.arange(m) < n
    x = np.where(np.arange(n) < m, 1.0, 3.0)
    lam = np.where(up, 2.0, 0.0)
    return Planted(np.eye(n), np.full(n, -3.0), A, b, x, lam, up.copy(), -np.ones(m, np.int64))


def planted_dense(n: int, m: int, seed: int, kind: str) -> Planted:
    """One QP of kind weak / dup / vertex / ties (module docstring):

    weak    k = max(1, min(n//3, m//3)) rows tight with integer lam* in [1, 4]
            and k more tight with lam* = 0; the 2k tight rows are independent
    dup     k = max(1, min(n//2, m//3)) independent tight rows with lam* > 0,
            each twice more among the rows: an exact copy and 2 x row with
            2 x b, both with lam* = 0 (`group` names the triples)
    vertex  min(m, n + max(1, n//2)) rows tight at x*, lam* > 0 on
            max(1, n//2) of them
    ties    _ties_dense; rows not permuted

    Non-tight rows get an integer slack in [1, 5]; the rows are permuted at
    the end so that tight rows land at arbitrary indices."""
    if kind == "ties":
        return _ties_dense(n, m)
    rs = np.random.default_rng([seed, n, m, _KIND_ID[kind]])
    H = _spd(rs, n)
    x = rs.integers(-3, 4, n).astype(np.float64)
    A, lam, tight, group = _plant_rows(rs, n, m, kind)
    b = A @ x + np.where(tight, 0.0, rs.integers(1, 6, m))
    f = -H @ x - A.T @ lam
    p = rs.permutation(m)
    return Planted(H, f, A[p], b[p], x, lam[p], tight[p], group[p])


def planted_eq(n: int, m: int, meq: int, seed: int, kind: str = "weak") -> Planted:
    """planted_dense's weak / dup on the rows >= meq only (k from n - meq and
    m - meq); rows 0 .. meq-1 are independent equalities, tight, with nonzero
    integer multipliers of both signs, and the tight rows that weak and dup
    call independent are independent of them too.  Only the inequality rows
    are permuted."""
    rs = np.random.default_rng([seed, n, m, meq, _KIND_ID[kind]])
    H = _spd(rs, n)
    x = rs.integers(-3, 4, n).astype(np.float64)
    E = _independent_rows(rs, meq, n)
    le = _mult(rs, meq) * np.where(np.arange(meq) % 2 == 0, 1.0, -1.0) * rs.choice([-1.0, 1.0])
    G, lam, tight, group = _plant_rows(rs, n, m - meq, kind, first=E)
    p = rs.permutation(m - meq)
    slack = np.where(tight, 0.0, rs.integers(1, 6, m - meq))
    A = np.concatenate([E, G[p]])
    lam = np.concatenate([le, lam[p]])
    b = A @ x + np.concatenate([np.zeros(meq), slack[p]])
    f = -H @ x - A.T @ lam
    return Planted(H, f, A, b, x, lam, np.concatenate([np.ones(meq, bool), tight[p]]),
                   np.concatenate([-np.ones(meq, np.int64), group[p]]))


def planted_box(n: int, seed: int, kind: str) -> PlantedBox:
    """One box QP, integer lb <= x* <= ub, H as planted_dense's:

    weak        a third of the variables on a bound with a multiplier in
                [1, 4], a third on a bound with a zero multiplier, the rest
                strictly inside
    pinned      lb_j == ub_j for a third of the variables with a planted
                integer mu_j of either sign (1 <= |mu_j| <= 4), a third
                strongly active on one bound, the rest strictly inside
    all_pinned  lb == ub everywhere (x* = lb), mu_j in [-4, 4], zero included
    ties        H = I, f = -3, the unit box: x* = 1, lam* = 2 on the upper bounds

    A third is max(1, n//3); which variables is a random choice."""
    I = np.eye(n)
    A = np.concatenate([I, -I])
    if kind == "ties":
        x, lam = np.ones(n), np.concatenate([np.full(n, 2.0), np.zeros(n)])
        lb, ub = -np.ones(n), np.ones(n)
        return PlantedBox(I, np.full(n, -3.0), lb, ub, x, lam, lam > 0, lam[:n] - lam[n:], np.zeros(n, bool),
                          np.ones(n, bool), A, np.concatenate([ub, -lb]))
    rs = np.random.default_rng([seed, n, _KIND_ID[kind]])
    H = _spd(rs, n)
    x = rs.integers(-3, 4, n).astype(np.float64)
    lb = x - rs.integers(1, 6, n)
    ub = x + rs.integers(1, 6, n)
    mu = np.zeros(n)
    pinned = np.zeros(n, bool)
    weak = np.zeros(n, bool)
    order = rs.permutation(n)
    k = max(1, n // 3)
    if kind == "all_pinned":
        first, second = order, order[:0]
    else:
        first, second = order[:k], order[k:2 * k]
    side = rs.choice([-1.0, 1.0], n)  # +1: the upper bound, -1: the lower
    if kind == "weak":
        strong, weakly = first, second
    elif kind in ("pinned", "all_pinned"):
        strong, weakly = second, order[:0]
        pinned[first] = True
        lb[first] = ub[first] = x[first]
        mu[first] = rs.integers(-4, 5, len(first)) if kind == "all_pinned" else _mult(rs, len(first)) * side[first]
    else:
        raise ValueError(kind)
    for j in np.concatenate([strong, weakly]).astype(int):
        if side[j] > 0:
            ub[j] = x[j]
        else:
            lb[j] = x[j]
    mu[strong] = _mult(rs, len(strong)) * side[strong]
    weak[weakly] = True
    lam = np.concatenate([np.maximum(mu, 0.0), np.maximum(-mu, 0.0)])
    f = -H @ x - mu
    tight = np.concatenate([ub == x, lb == x])
    return PlantedBox(H, f, lb, ub, x, lam, tight, mu, pinned, ~(pinned | weak), A, np.concatenate([ub, -lb]))


def batch_of(make, count: int, kinds, seed: int):
    """QP i = make(seed + i, kinds[i % len(kinds)]), stacked field by field:
    the kinds interleave, so a QP's partners in a wavefront differ from it."""
    qs = [make(seed + i, kinds[i % len(kinds)]) for i in range(count)]
    return type(qs[0])(*(np.stack(v) for v in zip(*qs))), [kinds[i % len(kinds)] for i in range(count)]


def dense_batch(n, m, count, kinds=DENSE_KINDS):
    return batch_of(lambda s, k: planted_dense(n, m, s, k), count, kinds, seed_of(n, m))


def eq_batch(n, m, meq, count, kinds=EQ_KINDS):
    return batch_of(lambda s, k: planted_eq(n, m, meq, s, k), count, kinds, seed_of(n, m) + meq)


def box_batch(n, count, kinds=BOX_KINDS):
    return batch_of(lambda s, k: planted_box(n, s, k), count, kinds, seed_of(n, 2 * n))


# ------------------------------------------------------------------ one-hot
class OneHot(NamedTuple):
    H: np.ndarray    # (n, n), shared
    f: np.ndarray    # (n,), shared
    A: np.ndarray    # (m, n), shared
    b: np.ndarray    # (Q, m): QP k's right-hand side
    x: np.ndarray    # (Q, n): closed form
    lam: np.ndarray  # (Q,): the multiplier of QP k's one active row
    row: np.ndarray  # (Q,): that row's index
    xu: np.ndarray   # (n,): the unconstrained minimiser

    def tiled(self):
        """(H, f, A, b) as a batch of Q QPs."""
        Q = len(self.b)
        return (np.broadcast_to(self.H, (Q,) + self.H.shape).copy(), np.broadcast_to(self.f, (Q, len(self.f))).copy(),
                np.broadcast_to(self.A, (Q,) + self.A.shape).copy(), self.b.copy())

    def mask(self):
        out = np.zeros(self.b.shape, bool)
        out[np.arange(len(self.row)), self.row] = True
        return out


MIN_SLACK = 0.5  # what every other row must keep at the closed-form x


def _one_hot_common(n, seed):
    rs = np.random.default_rng(seed)
    B = rs.standard_normal((n, n))
    H = np.eye(n) + B.T @ B / n
    f = 3.0 * rs.standard_normal(n)
    return rs, H, f, np.linalg.solve(H, -f)


def _one_hot_finish(H, f, A, b, x, lam, rows, xu, free=None):
    """The precondition: at the closed-form x every row but the active one (and
    the equalities, `free` = first inequality row) keeps slack > MIN_SLACK."""
    s = b - x @ A.T
    s[np.arange(len(rows)), rows] = np.inf
    if free:
        s[:, :free] = np.inf
    assert s.min() > MIN_SLACK, ("one-hot precondition", float(s.min()))
    assert (lam > 0).all()
    return OneHot(H, f, A, b, x, lam, np.asarray(rows), xu)


def one_hot_rows(n: int, m: int, seed: int, slack: float = 4.0) -> OneHot:
    """m QPs sharing H = I + B^T B / n (B ~ N(0, 1)), f ~ 3 N(0, 1) and m
    unit-norm random rows.  With xu = -H^{-1} f, QP k has b = A xu + slack but
    b_k = a_k xu - 1: row k alone is violated at xu, and
        lam_k = 1 / (a_k H^{-1} a_k),  x = xu - lam_k H^{-1} a_k,
    active set {k}."""
    rs, H, f, xu = _one_hot_common(n, seed)
    A = rs.standard_normal((m, n))
    A /= np.linalg.norm(A, axis=1, keepdims=True)
    W = np.linalg.solve(H, A.T)                  # H^{-1} a_k in column k
    lam = 1.0 / np.einsum("kj,jk->k", A, W)
    b = np.tile(A @ xu + slack, (m, 1))
    b[np.arange(m), np.arange(m)] = A @ xu - 1.0
    x = xu[None, :] - lam[:, None] * W.T
    return _one_hot_finish(H, f, A, b, x, lam, np.arange(m), xu)


def one_hot_bounds(n: int, seed: int, slack: float = 4.0):
    """one_hot_rows for qpb_solve_box: 2n QPs, QP j violates only upper bound j
    (ub_j = xu_j - 1) and QP n + j only lower bound j (lb_j = xu_j + 1); the
    other bounds are xu -+ slack.  Returns (OneHot on A = [I; -I], b = [ub;
    -lb], lb (2n, n), ub (2n, n)); row k of the mask is bit k in qpb.h's
    upper-then-lower order."""
    rs, H, f, xu = _one_hot_common(n, seed)
    A = np.concatenate([np.eye(n), -np.eye(n)])
    ub = np.tile(xu + slack, (2 * n, 1))
    lb = np.tile(xu - slack, (2 * n, 1))
    j = np.arange(n)
    ub[j, j] = xu - 1.0
    lb[n + j, j] = xu + 1.0
    W = np.linalg.solve(H, A.T)
    lam = 1.0 / np.einsum("kj,jk->k", A, W)
    x = xu[None, :] - lam[:, None] * W.T
    return _one_hot_finish(H, f, A, np.concatenate([ub, -lb], axis=1), x, lam, np.arange(2 * n), xu), lb, ub


def one_hot_eq(n: int, m: int, meq: int, seed: int, slack: float = 4.0):
    """one_hot_rows with rows 0 .. meq-1 equalities that are tight at xu
    (b_i = a_i xu): they are taken with a zero multiplier and move nothing.
    m - meq QPs; QP k violates inequality row meq + k alone.  The closed form
    is the projection inside null(E), Z an orthonormal basis of it:
        ar = Z^T a,  Hr = Z^T H Z,  lam = 1 / (ar Hr^{-1} ar),
        x = xu - lam Z Hr^{-1} ar
    Returns (OneHot, lam_eq (Q, meq)), lam_eq from stationarity."""
    rs, H, f, xu = _one_hot_common(n, seed)
    A = rs.standard_normal((m, n))
    A /= np.linalg.norm(A, axis=1, keepdims=True)
    E = A[:meq]
    Z = np.linalg.qr(E.T, mode="complete")[0][:, meq:]
    G = A[meq:]
    W = Z @ np.linalg.solve(Z.T @ H @ Z, Z.T @ G.T)
    lam = 1.0 / np.einsum("kj,jk->k", G, W)
    Q = m - meq
    b = np.tile(A @ xu + slack, (Q, 1))
    b[:, :meq] = E @ xu
    rows = meq + np.arange(Q)
    b[np.arange(Q), rows] = G @ xu - 1.0
    x = xu[None, :] - lam[:, None] * W.T
    assert np.abs(x @ E.T - b[:, :meq]).max() <= 1e-12
    lam_eq = np.linalg.lstsq(E.T, -(H @ x.T + f[:, None] + G.T * lam[None, :]), rcond=None)[0].T
    return _one_hot_finish(H, f, A, b, x, lam, rows, xu, free=meq), lam_eq
