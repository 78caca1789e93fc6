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
    planted_range, planted_range_shared
                   weak / dup / vertex / pinned / thin     bl <= A x <= bu
    planted_range_box
                   weak / pinned / vertex / dup_bound      bl <= G x <= bu, lb <= x <= ub
    one_hot_range  2 (m - meq) QPs: every row the one active row on each side

In the range families lam* is signed as qpb_solve_range defines it
(H x + f + A^T lam = 0: negative at a lower bound) and `side` says where a row
sits at x*: +1 tight at bu only, -1 tight at bl only, 2 zero width
(bl == bu == a x*; the equalities are 2), 0 slack on both sides.

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
# (n, m, meq, batch): the RG forms of gi_dense (one and two rows per lane padded, n = 16 at one row per lane, full)
# and of gi_wave (m = 33 at n = 16: the class edge; padded; full).  At (16, 16, 0) m - meq == n - meq, so a `vertex`
# QP cannot have more tight rows than n - meq: all 16 rows are tight there and half carry no multiplier, which is
# degenerate only in the weak sense; every other route has tight > n - meq (tests/test_planted.py)
RANGE = [(7, 14, 2, 37), (13, 26, 3, 37), (16, 16, 0, 37), (16, 32, 4, 37), (16, 33, 0, 13), (20, 33, 5, 13),
         (32, 64, 8, 13)]
# (n, mg, meq, batch): the BX forms, m = mg + n rows of which the last n are made in registers
RANGE_BOX = [(7, 7, 0, 37), (12, 20, 3, 37), (16, 16, 2, 37), (16, 0, 0, 13), (16, 17, 1, 13), (20, 9, 0, 13),
             (32, 32, 3, 13), (32, 0, 0, 13)]
# (n, m, meq, batch): the SH and factored forms' shared batches
RANGE_SHARED = [(16, 32, 4, 13), (20, 33, 5, 13)]

DENSE_KINDS = ("weak", "dup", "vertex")
EQ_KINDS = ("weak", "dup")
BOX_KINDS = ("weak", "pinned", "all_pinned")
RANGE_KINDS = ("weak", "dup", "vertex", "pinned")
RANGE_SHARED_KINDS = ("weak", "vertex", "thin")
RANGE_BOX_KINDS = ("weak", "pinned", "vertex", "dup_bound")
_KIND_ID = {"weak": 1, "dup": 2, "vertex": 3, "pinned": 4, "all_pinned": 5, "thin": 6, "dup_bound": 7}


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


# ------------------------------------------------------------ range families
THIN = 2.0 ** -20  # the width of a `thin` row: far above the feasibility tolerance, far below every other slack


class PlantedRange(NamedTuple):
    H: np.ndarray
    f: np.ndarray
    A: np.ndarray
    bl: np.ndarray
    bu: np.ndarray
    x: np.ndarray      # x*
    lam: np.ndarray    # lam*, signed: H x + f + A^T lam = 0, negative at a lower bound
    side: np.ndarray   # int: +1 tight at bu only, -1 tight at bl only, 2 zero width, 0 slack on both sides
    group: np.ndarray  # int: the set of dependent rows (dup triple, pinned pair, dup_bound pair) a row is in, or -1


class PlantedRangeBox(NamedTuple):
    H: np.ndarray
    f: np.ndarray
    G: np.ndarray      # (mg, n), mg = 0 allowed
    bl: np.ndarray
    bu: np.ndarray
    lb: np.ndarray
    ub: np.ndarray
    x: np.ndarray
    lam_g: np.ndarray  # (mg,) signed
    mu: np.ndarray     # (n,) signed: > 0 at ub, < 0 at lb
    pinned: np.ndarray  # (n,) bool: lb_j == ub_j
    # the materialised problem, range_box_oracle.materialise's order: [G; I], [bl; lb], [bu; ub]
    A: np.ndarray
    lo: np.ndarray
    hi: np.ndarray
    lam: np.ndarray
    side: np.ndarray
    group: np.ndarray

    def materialised(self) -> PlantedRange:
        return PlantedRange(self.H, self.f, self.A, self.lo, self.hi, self.x, self.lam, self.side, self.group)


def _signs(rs, k):
    return rs.choice([-1, 1], k)


def _plant_range_rows(rs, n, mi, kind, first):
    """The rows >= meq of one range QP before the permutation: (G, lam, side,
    group), tight rows first.  `first`: the rows (equalities, tight variable
    bounds) that the tight rows called independent are independent of too."""
    nf = n - len(first)
    G = _rows(rs, mi, n)
    lam = np.zeros(mi)
    side = np.zeros(mi, np.int64)
    group = -np.ones(mi, np.int64)
    if mi == 0:
        return G, lam, side, group
    k3 = max(1, min(nf // 3, mi // 3))
    if kind == "weak":
        k = k3
        G[:2 * k] = _independent_rows(rs, 2 * k, n, first)
        side[:2 * k] = _signs(rs, 2 * k)
        lam[:k] = _mult(rs, k) * side[:k]
    elif kind == "dup":
        k = max(1, min(nf // 2, mi // 3))
        G[:k] = _independent_rows(rs, k, n, first)
        G[k:2 * k] = -G[:k]          # the same half-space held in the other orientation
        G[2 * k:3 * k] = 2.0 * G[:k]
        s = _signs(rs, k)
        side[:3 * k] = np.concatenate([s, -s, s])
        lam[:k] = _mult(rs, k) * s
        group[:3 * k] = np.tile(np.arange(k), 3)
    elif kind == "vertex":
        p = max(1, nf // 2)
        t = min(mi, nf + p)
        side[:t] = _signs(rs, t)
        lam[:p] = _mult(rs, p) * side[:p]
    elif kind == "pinned":
        k = k3
        G[:k] = _independent_rows(rs, k, n, first)
        G[k:2 * k] = G[:k]
        side[:2 * k] = 2
        lam[:k] = _mult(rs, k) * _signs(rs, k)
        group[:2 * k] = np.tile(np.arange(k), 2)
    elif kind == "thin":
        k = max(1, min(nf // 2, mi // 2))
        G[:k] = _independent_rows(rs, k, n, first)
        side[:k] = _signs(rs, k)
        lam[:k] = _mult(rs, k) * side[:k]
    else:
        raise ValueError(kind)
    return G, lam, side, group


def _range_bounds(rs, ax, side, thin=False):
    """(bl, bu) around the exact row values ax: a tight side sits on ax, the
    other side of a tight row an integer in [1, 5] (THIN for `thin`) away; a
    slack row gets integer slacks in [1, 5] on both sides, about a third of
    them bl = -inf and about a third bu = +inf."""
    k = len(ax)
    below = rs.integers(1, 6, k).astype(np.float64)
    above = rs.integers(1, 6, k).astype(np.float64)
    absent = rs.integers(0, 3, k)
    if thin:
        below[side != 0] = above[side != 0] = THIN
    bl = np.where((side == -1) | (side == 2), ax, ax - below)
    bu = np.where((side == 1) | (side == 2), ax, ax + above)
    bl[(side == 0) & (absent == 0)] = -np.inf
    bu[(side == 0) & (absent == 1)] = np.inf
    return bl, bu


def _equalities(rs, meq, n):
    """planted_eq's: independent rows, nonzero integer multipliers of both signs."""
    if meq == 0:
        return np.zeros((0, n)), np.zeros(0)
    E = _independent_rows(rs, meq, n)
    le = _mult(rs, meq) * np.where(np.arange(meq) % 2 == 0, 1.0, -1.0) * rs.choice([-1.0, 1.0])
    return E, le


def planted_range(n: int, m: int, meq: int, seed: int, kind: str) -> PlantedRange:
    """One QP bl <= A x <= bu whose rows < meq are planted_eq's equalities
    (bl = bu, side 2) and whose rows >= meq are, with nf = n - meq, mi = m - meq:

    weak    k = max(1, min(nf//3, mi//3)) rows tight with |lam*| in [1, 4] and
            k more tight with lam* = 0, each on a random side; the 2k tight
            rows are independent of each other and of the equalities
    dup     k = max(1, min(nf//2, mi//3)) independent tight rows a with
            lam* != 0 on a random side, each twice more with lam* = 0: the
            negated row -a tight on the opposite side, and 2a with its bounds
            scaled by 2, tight on the same side (`group` names the triples)
    vertex  min(mi, nf + max(1, nf//2)) rows tight on random sides, lam* != 0
            on max(1, nf//2) of them with the sign its side names
    pinned  k (weak's) independent zero-width rows with integer multipliers of
            either sign, each a second time as an exact copy with lam* = 0
            (`group` names the pairs)
    thin    not degenerate: k = max(1, min(nf//2, mi//2)) independent rows
            tight on a random side with lam* != 0, the opposite bound exactly
            THIN = 2^-20 away; the active set is unique

    The bounds are _range_bounds'; only the rows >= meq are permuted."""
    rs = np.random.default_rng([seed, n, m, meq, 16 + _KIND_ID[kind]])
    H = _spd(rs, n)
    x = rs.integers(-3, 4, n).astype(np.float64)
    E, le = _equalities(rs, meq, n)
    G, lam, side, group = _plant_range_rows(rs, n, m - meq, kind, E)
    bl, bu = _range_bounds(rs, G @ x, side, thin=kind == "thin")
    if kind == "dup":  # the copies describe the first row's range: [-bu, -bl] for -a, [2 bl, 2 bu] for 2a
        k = int((group >= 0).sum()) // 3
        bl[k:2 * k], bu[k:2 * k] = -bu[:k], -bl[:k]
        bl[2 * k:3 * k], bu[2 * k:3 * k] = 2.0 * bl[:k], 2.0 * bu[:k]
    p = rs.permutation(m - meq)
    A = np.concatenate([E, G[p]])
    lam = np.concatenate([le, lam[p]])
    f = -H @ x - A.T @ lam
    return PlantedRange(H, f, A, np.concatenate([E @ x, bl[p]]), np.concatenate([E @ x, bu[p]]), x, lam,
                        np.concatenate([np.full(meq, 2), side[p]]), np.concatenate([-np.ones(meq, np.int64), group[p]]))


def range_rank_required(kind: str, n: int, meq: int, tight: int) -> int:
    """rank([E; A_tight]) that a kind claims, `tight` counting the equalities:
    full row rank for weak and thin, min(tight, n) for vertex."""
    return min(tight, n) if kind == "vertex" else tight


def planted_range_shared(n: int, m: int, meq: int, count: int, seed: int):
    """One H and one A = [E; G] for `count` QPs (the factored and SH forms'
    batch): QP i has kind RANGE_SHARED_KINDS[i % 3] with its own x*, tight rows
    of G (a random choice, redrawn until rank([E; A_tight]) is what the kind
    requires, range_rank_required), sides and lam*.  Returns (PlantedRange with
    H and A repeated along the batch axis, kinds)."""
    rs = np.random.default_rng([seed, n, m, meq, count, 0x5A])
    H = _spd(rs, n)
    E = _independent_rows(rs, meq, n)
    A = np.concatenate([E, _rows(rs, m - meq, n)])
    mi, nf = m - meq, n - meq
    qs, kinds = [], []
    for i in range(count):
        kind = RANGE_SHARED_KINDS[i % len(RANGE_SHARED_KINDS)]
        p = max(1, nf // 2)
        if kind == "weak":
            k = max(1, min(nf // 3, mi // 3))
            t, nz = 2 * k, k
        elif kind == "vertex":
            t, nz = min(mi, nf + p), p
        else:
            t = nz = max(1, min(nf // 2, mi // 2))
        while True:
            rows = meq + rs.permutation(mi)[:t]
            if np.linalg.matrix_rank(np.concatenate([E, A[rows]])) == range_rank_required(kind, n, meq, meq + t):
                break
        x = rs.integers(-3, 4, n).astype(np.float64)
        side = np.concatenate([np.full(meq, 2), np.zeros(mi, np.int64)])
        side[rows] = _signs(rs, t)
        lam = np.zeros(m)
        lam[:meq] = _mult(rs, meq) * np.where(np.arange(meq) % 2 == 0, 1.0, -1.0) * rs.choice([-1.0, 1.0])
        lam[rows[:nz]] = _mult(rs, nz) * side[rows[:nz]]
        bl, bu = _range_bounds(rs, A @ x, side, thin=kind == "thin")
        qs.append(PlantedRange(H, -H @ x - A.T @ lam, A, bl, bu, x, lam, side, -np.ones(m, np.int64)))
        kinds.append(kind)
    return PlantedRange(*(np.stack(v) for v in zip(*qs))), kinds


def planted_range_box(n: int, mg: int, meq: int, seed: int, kind: str) -> PlantedRangeBox:
    """One QP bl <= G x <= bu, lb <= x <= ub with f = -H x* - G^T lam_G - mu.
    The variable bounds are planted_box's, with kb = max(1, (n - meq)//6):

    weak, vertex  kb variables on a bound with |mu| in [1, 4], kb on a bound
                  with mu = 0, the rest strictly inside
    pinned        kb variables with lb_j == ub_j and an integer mu_j of either
                  sign, kb strongly active on one bound, kb on a bound with
                  mu = 0 (a zero-width row is ONE row here, not a dependent pair)
    dup_bound     kd = max(1, min(n//4, (mg - meq)//2)) variables on a bound
                  with mu != 0, each beside a G row e_j or 2 e_j (alternating)
                  that is tight on the same side with lam* = 0: a loaded row
                  that depends on a register-made one (`group` names the
                  pairs); kb more variables strongly active alone

    The G rows are planted_range's of the same kind (dup_bound: its pairs, the
    other rows slack) with the tight variable bounds counted among the rows
    that tight rows are independent of, so nf = n - meq - (tight bounds).
    A variable on one bound has its other bound THIN = 2^-20 away: x0 - x* is
    small on a variable with mu = 0 (H^-1 spreads the multipliers thinly, and
    with mg = 0 only through H's off-diagonal), so only a narrow range puts the
    unconstrained minimiser beyond the far bound -- about half of the weakly
    active variables are then violated at x0 on the side opposite to the one
    they end on, and a register-made row must reach a flip
    (tests/test_planted.py asserts the counts).  Variables strictly inside get
    integer slacks in [1, 5], about a third of them lb = -inf and about a
    third ub = +inf.  Needs mg = 0 or mg - meq >= 3
    (dup_bound: mg - meq >= 1)."""
    rs = np.random.default_rng([seed, n, mg, meq, 32 + _KIND_ID[kind]])
    mi = mg - meq
    H = _spd(rs, n)
    x = rs.integers(-3, 4, n).astype(np.float64)
    E, le = _equalities(rs, meq, n)
    order = rs.permutation(n)
    kb = max(1, (n - meq) // 6)
    kd = max(1, min(n // 4, mi // 2)) if kind == "dup_bound" else 0
    vside = np.zeros(n, np.int64)
    mu = np.zeros(n)
    strong, second, dup = order[:kb], order[kb:2 * kb], order[2 * kb:2 * kb + kd]
    vside[strong] = _signs(rs, kb)
    mu[strong] = _mult(rs, kb) * vside[strong]
    if kind in ("weak", "vertex"):
        vside[second] = _signs(rs, kb)
    elif kind == "pinned":
        vside[second] = 2
        mu[second] = _mult(rs, kb) * _signs(rs, kb)
        vside[order[2 * kb:3 * kb]] = _signs(rs, kb)
    elif kind == "dup_bound":
        assert mi >= kd >= 1, (mg, meq)
        vside[dup] = _signs(rs, kd)
        mu[dup] = _mult(rs, kd) * vside[dup]
    else:
        raise ValueError(kind)
    lb, ub = _range_bounds(rs, x, vside, thin=True)
    first = np.concatenate([E, np.eye(n)[vside != 0]])
    if kind == "dup_bound":
        G, lam_g, side, group = _rows(rs, mi, n), np.zeros(mi), np.zeros(mi, np.int64), -np.ones(mi, np.int64)
        G[:kd] = np.eye(n)[dup] * np.where(np.arange(kd) % 2 == 0, 1.0, 2.0)[:, None]
        side[:kd] = vside[dup]
        group[:kd] = np.arange(kd)
    else:
        G, lam_g, side, group = _plant_range_rows(rs, n, mi, kind, first)
    bl, bu = _range_bounds(rs, G @ x, side)
    p = rs.permutation(mi)
    G = np.concatenate([E, G[p]])
    bl, bu = np.concatenate([E @ x, bl[p]]), np.concatenate([E @ x, bu[p]])
    lam_g = np.concatenate([le, lam_g[p]])
    side = np.concatenate([np.full(meq, 2), side[p]])
    vgroup = -np.ones(n, np.int64)
    vgroup[dup] = np.arange(kd)
    f = -H @ x - G.T @ lam_g - mu
    return PlantedRangeBox(H, f, G, bl, bu, lb, ub, x, lam_g, mu, vside == 2,
                           np.concatenate([G, np.eye(n)]), np.concatenate([bl, lb]), np.concatenate([bu, ub]),
                           np.concatenate([lam_g, mu]), np.concatenate([side, vside]),
                           np.concatenate([-np.ones(meq, np.int64), group[p], vgroup]))


RANGE_SEED_SHIFT = 8  # see range_batch


def range_batch(n, m, meq, count, kinds=RANGE_KINDS):
    """QP i has kind kinds[i % len(kinds)] and seed seed_of(n, m) + meq + 8 + i.
    The shift 8 is the first at which, on every RANGE route, the interleaved
    batch, its first six QPs (solved one at a time from a factor buffer) and
    the three `thin` QPs each have rows that are tight on the side opposite to
    the one violated at x0 (opposite_side_rows), for weak and for vertex
    separately; tests/test_planted.py asserts it."""
    return batch_of(lambda s, k: planted_range(n, m, meq, s, k), count, kinds,
                    seed_of(n, m) + meq + RANGE_SEED_SHIFT)


def range_shared_batch(n, m, meq, count):
    return planted_range_shared(n, m, meq, count, seed_of(n, m) + meq)


def range_box_kinds(mg, meq):
    """dup_bound needs a G row beyond the equalities."""
    return RANGE_BOX_KINDS if mg - meq >= 1 else RANGE_BOX_KINDS[:3]


def range_box_batch(n, mg, meq, count):
    return batch_of(lambda s, k: planted_range_box(n, mg, meq, s, k), count, range_box_kinds(mg, meq),
                    seed_of(n, mg + n) + meq)


def opposite_side_rows(q: PlantedRange, meq: int) -> np.ndarray:
    """Per QP of a batch: the rows >= meq that are tight on one side at x* and
    violated on the OTHER side at the unconstrained minimiser x0 = -H^-1 f.
    A kernel that starts from x0 holds such a row on the wrong side first: it
    must reach a flip (or a DROP and a return on the other side)."""
    x0 = -np.linalg.solve(q.H, q.f[:, :, None])[:, :, 0]
    a0 = np.einsum("bij,bj->bi", q.A, x0)
    opp = ((q.side == 1) & (a0 < q.bl)) | ((q.side == -1) & (a0 > q.bu))
    return opp[:, meq:].sum(axis=1)


class OneHotRange(NamedTuple):
    H: np.ndarray       # (n, n), shared
    f: np.ndarray       # (n,), shared
    A: np.ndarray       # (m, n), shared; the last box_rows rows are the identity
    bl: np.ndarray      # (Q, m)
    bu: np.ndarray      # (Q, m)
    x: np.ndarray       # (Q, n): closed form
    lam: np.ndarray     # (Q,): the signed multiplier of QP k's one active row
    row: np.ndarray     # (Q,): that row's index
    lower: np.ndarray   # (Q,) bool: the row sits at its lower bound (the second half)
    lam_eq: np.ndarray  # (Q, meq): the equalities' multipliers, from stationarity
    xu: np.ndarray      # (n,)

    def tiled(self):
        """(H, f, A, bl, bu) as a batch of Q QPs."""
        Q = len(self.bl)
        return (np.broadcast_to(self.H, (Q,) + self.H.shape).copy(), np.broadcast_to(self.f, (Q, len(self.f))).copy(),
                np.broadcast_to(self.A, (Q,) + self.A.shape).copy(), self.bl.copy(), self.bu.copy())

    def mask(self):
        out = np.zeros(self.bl.shape, bool)
        out[np.arange(len(self.row)), self.row] = True
        return out


def one_hot_range(n: int, m: int, meq: int, seed: int, box_rows: int = 0, slack: float = 4.0) -> OneHotRange:
    """one_hot_eq for qpb_solve_range: 2 (m - meq) QPs sharing H, f and A
    (unit-norm random rows; the last `box_rows` rows are the last rows of the
    identity, for the range-box form).  The equalities are tight at xu.  Every
    bound is A xu -+ slack except one: QP k has bu_k = a_k xu - 1 on row
    meq + k (its upper side alone is violated at xu) and QP (m - meq) + k has
    bl_k = a_k xu + 1 (its lower side alone).  The closed form is one_hot_eq's
    with the signed multiplier:
        lam = +-1 / (ar Hr^{-1} ar),  x = xu - lam Z Hr^{-1} ar
    (+ at the upper bound, - at the lower).  At the closed-form x every other
    row, and the active row's other side, keeps MIN_SLACK on both sides."""
    rs, H, f, xu = _one_hot_common(n, seed)
    A = rs.standard_normal((m, n))
    A /= np.linalg.norm(A, axis=1, keepdims=True)
    if box_rows:
        A[m - box_rows:] = np.eye(n)[n - box_rows:]
    E, G = A[:meq], A[meq:]
    Z = np.linalg.qr(E.T, mode="complete")[0][:, meq:] if meq else np.eye(n)
    W = Z @ np.linalg.solve(Z.T @ H @ Z, Z.T @ G.T)
    K = m - meq
    mag = 1.0 / np.einsum("kj,jk->k", G, W)
    assert (mag > 0).all()
    lam = np.concatenate([mag, -mag])
    rows = meq + np.concatenate([np.arange(K), np.arange(K)])
    lower = np.arange(2 * K) >= K
    bu = np.tile(A @ xu + slack, (2 * K, 1))
    bl = np.tile(A @ xu - slack, (2 * K, 1))
    bl[:, :meq] = bu[:, :meq] = E @ xu
    k = np.arange(K)
    bu[k, meq + k] = G @ xu - 1.0
    bl[K + k, meq + k] = G @ xu + 1.0
    x = xu[None, :] - lam[:, None] * np.concatenate([W.T, W.T])
    assert meq == 0 or np.abs(x @ E.T - bu[:, :meq]).max() <= 1e-12
    lam_eq = np.zeros((2 * K, 0))
    if meq:
        lam_eq = np.linalg.lstsq(E.T, -(H @ x.T + f[:, None] + G.T[:, rows - meq] * lam[None, :]), rcond=None)[0].T
    ax = x @ A.T
    su, sl = bu - ax, ax - bl
    q = np.arange(2 * K)
    su[q[~lower], rows[~lower]] = np.inf  # the active side itself
    sl[q[lower], rows[lower]] = np.inf
    su[:, :meq] = sl[:, :meq] = np.inf
    assert min(su.min(), sl.min()) > MIN_SLACK, ("one-hot precondition", float(su.min()), float(sl.min()))
    return OneHotRange(H, f, A, bl, bu, x, lam, rows, lower, lam_eq, xu)
