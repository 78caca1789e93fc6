"""oracle/oracle.py -- TEST INFRASTRUCTURE ONLY (the checker, never the product).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import
this module.  Nothing here is on the product path; the product is the HIP
library under embedded-qp-solver_amd/.

CPU restatement (numpy) of the reference behaviour on the hot path:

* glibc ``rand()`` (TYPE_3 additive-feedback generator) -- the reference seeds
  it with ``srand`` (main.c:11) and draws every input through it
  (matrix_ops.c:677-681).  Restated so inputs are reproducible without the
  reference build.
* the reference input generator: ``random_number`` (matrix_ops.c:677-681),
  ``matrix_random`` (:683-697, row-major draws), ``matirx_random_pos_def``
  (:699-734: B random, P = B^T B by the sequential-k ``matrix_mult``
  (:235-271), then scaled by 1/(max*nrows)), in the P, q, x0 order of
  main.c:37-39.
* ``test/qp_ref.py``: reads the wire format (qp_ref.py:8-30, written by
  test/test.c:108-126) and solves ``solve_qp(P, q, G=0, h=0)`` (qp_ref.py:35),
  i.e. the unconstrained minimiser x* = -P^{-1} q, printing
  eval_qp = 1/2 x^T P x + q^T x (qp_ref.py:5-6).  ``qpsolvers`` is absent from
  the image and unpinned, so it is restated as a dense solve.
* constrained oracle (north_star's active-set path has NO reference
  implementation -- SURVEY.md §0/§8c): a primal active-set method
  (Nocedal & Wright, Numerical Optimization, 2nd ed., Alg. 16.3) for
  min 1/2 x^T H x + f^T x  s.t.  A x <= b, written independently of the GPU's
  dual (Goldfarb-Idnani) method, plus a KKT certificate.  Parity for this row
  is pinned by the certificate, not by a reference output.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass

import numpy as np

RAND_MAX = 2147483647

# --------------------------------------------------------------------------
# glibc rand() restatement (TYPE_3, degree 31, separation 3)
# --------------------------------------------------------------------------


class GlibcRand:
    """Restatement of glibc's srand/rand (stdlib/random_r.c, TYPE_3).

    r[0] = seed; r[i] = 16807 * r[i-1] mod (2^31-1) for i < 31;
    r[i] = r[i-31] + r[i-3] (mod 2^32) afterwards; the first 310 outputs of
    the feedback loop are discarded and rand() returns r[i] >> 1.
    """

    def __init__(self, seed: int = 1):
        self.seed(seed)

    def seed(self, seed: int) -> None:
        seed &= 0xFFFFFFFF
        if seed >= 0x80000000:
            seed -= 0x100000000  # stored as int32_t
        if seed == 0:
            seed = 1
        r = [0] * 34
        r[0] = seed
        for i in range(1, 31):
            hi, lo = divmod(r[i - 1], 127773) if r[i - 1] >= 0 else (
                -((-r[i - 1]) // 127773), -((-r[i - 1]) % 127773))
            word = 16807 * lo - 2836 * hi
            if word < 0:
                word += 2147483647
            r[i] = word
        for i in range(31, 34):
            r[i] = r[i - 31]
        self._r = [x & 0xFFFFFFFF for x in r]
        # discard 310 outputs (glibc srandom_r: 10 * rand_deg)
        for _ in range(310):
            self._next()

    def _next(self) -> int:
        r = self._r
        v = (r[-31] + r[-3]) & 0xFFFFFFFF
        r.append(v)
        if len(r) > 64:
            del r[:-34]
        return v >> 1

    def rand(self) -> int:
        return self._next()

    def rand_array(self, count: int) -> np.ndarray:
        return np.array([self._next() for _ in range(count)], dtype=np.float64)


def random_number(rng: GlibcRand, lo: float, hi: float, count: int) -> np.ndarray:
    """matrix_ops.c:677-681: min + r * (max - min) / RAND_MAX (left-to-right)."""
    r = rng.rand_array(count)
    return lo + (r * (hi - lo)) / RAND_MAX


def ref_random_pos_def(rng: GlibcRand, n: int, lo: float = -1e3, hi: float = 1e3) -> np.ndarray:
    """matrix_ops.c:699-734 with the sequential-k matrix_mult of :235-271."""
    B = random_number(rng, lo, hi, n * n).reshape(n, n)  # matrix_random: row-major
    acc = np.zeros((n, n))
    for k in range(n):  # P[i][j] = sum_k B^T[i][k] * B[k][j], k ascending, no FMA
        acc = acc + np.outer(B[k, :], B[k, :])
    scale = 1.0 / float(hi * n)
    return acc * scale


def ref_generate(seed: int, count: int, n: int, prange=(-1e3, 1e3), qrange=(-1e3, 1e3),
                 xrange=(-1e3, 1e3)):
    """count QPs in main.c:37-39 order (P, q, x0) after srand(seed)."""
    rng = GlibcRand(seed)
    P = np.empty((count, n, n))
    q = np.empty((count, n))
    x0 = np.empty((count, n))
    for i in range(count):
        P[i] = ref_random_pos_def(rng, n, *prange)
        q[i] = random_number(rng, *qrange, n)
        x0[i] = random_number(rng, *xrange, n)
    return P, q, x0


# --------------------------------------------------------------------------
# wire format (test/test.c:108-126 writer, test/qp_ref.py:8-30 reader)
# --------------------------------------------------------------------------


def write_wire(path: str, P: np.ndarray, q: np.ndarray) -> None:
    """[n as double][P row-major n*n][q n], native-endian fp64 (test.c:110-121)."""
    n = P.shape[0]
    with open(path, "wb") as fp:
        fp.write(struct.pack("d", float(n)))
        fp.write(np.ascontiguousarray(P, dtype=np.float64).tobytes())
        fp.write(np.ascontiguousarray(q, dtype=np.float64).reshape(n).tobytes())


def read_wire(path: str):
    """qp_ref.py:8-30: returns (n, P (n,n), q (n,))."""
    with open(path, "rb") as fp:
        data = fp.read()
    vals = np.frombuffer(data, dtype=np.float64)
    n = int(vals[0])
    P = vals[1:1 + n * n].reshape(n, n).copy()
    q = vals[1 + n * n:1 + n * n + n].copy()
    return n, P, q


def write_wire_batch(path: str, H: np.ndarray, f: np.ndarray, A=None, b=None) -> None:
    """Batched wire form: fp64 [n][m][B] then B records [H][f][A][b]
    (csrc/qpb_wire.c; the reference form when m == 0 and B == 1)."""
    B, n = f.shape
    m = 0 if A is None else A.shape[1]
    if m == 0 and B == 1:
        write_wire(path, H[0], f[0])
        return
    recs = [np.asarray(H, np.float64).reshape(B, -1), np.asarray(f, np.float64).reshape(B, -1)]
    if m:
        recs += [np.asarray(A, np.float64).reshape(B, -1), np.asarray(b, np.float64).reshape(B, -1)]
    with open(path, "wb") as fp:
        fp.write(np.array([n, m, B], dtype=np.float64).tobytes())
        fp.write(np.concatenate(recs, axis=1).tobytes())


def read_wire_batch(path: str):
    """Either wire form -> (H (B,n,n), f (B,n), A (B,m,n), b (B,m))."""
    vals = np.fromfile(path, dtype=np.float64)
    n = int(vals[0])
    if vals.size == 1 + n * n + n:
        _, P, q = read_wire(path)
        return P[None], q[None], np.zeros((1, 0, n)), np.zeros((1, 0))
    m, B = int(vals[1]), int(vals[2])
    rec = vals[3:].reshape(B, n * n + n + m * n + m)
    H = rec[:, :n * n].reshape(B, n, n)
    f = rec[:, n * n:n * n + n]
    A = rec[:, n * n + n:n * n + n + m * n].reshape(B, m, n)
    b = rec[:, n * n + n + m * n:]
    return H.copy(), f.copy(), A.copy(), b.copy()


def eval_qp(P, q, x):
    """qp_ref.py:5-6 (no constant term)."""
    return 0.5 * x @ P @ x + q @ x


def qp_ref_solve(P, q):
    """qp_ref.py:35 with G=0, h=0: the constraint 0 <= 0 is vacuous, so the
    solution is the unconstrained minimiser -P^{-1} q."""
    return np.linalg.solve(P, -q)


# --------------------------------------------------------------------------
# constrained oracle: primal active set (Nocedal & Wright Alg. 16.3)
# --------------------------------------------------------------------------


@dataclass
class ASResult:
    x: np.ndarray
    lam: np.ndarray
    active: np.ndarray  # bool (m,)
    iters: int
    status: int  # 0 ok, 1 max-iter, 3 infeasible start


def _eqp(H, g, Aw):
    n = H.shape[0]
    k = Aw.shape[0]
    if k == 0:
        return np.linalg.solve(H, -g), np.zeros(0)
    K = np.zeros((n + k, n + k))
    K[:n, :n] = H
    K[:n, n:] = Aw.T
    K[n:, :n] = Aw
    rhs = np.concatenate([-g, np.zeros(k)])
    sol = np.linalg.solve(K, rhs)
    return sol[:n], sol[n:]


def active_set_solve(H, f, A, b, x0=None, max_iter=500, tol=1e-11) -> ASResult:
    """min 1/2 x^T H x + f^T x  s.t.  A x <= b  (H SPD), from a feasible x0.

    Lagrangian convention: H x + f + A^T lam = 0, lam >= 0,
    lam_i (b_i - a_i^T x) = 0.
    """
    H = np.asarray(H, float)
    f = np.asarray(f, float)
    A = np.asarray(A, float).reshape(-1, H.shape[0])
    b = np.asarray(b, float).reshape(-1)
    n, m = H.shape[0], A.shape[0]
    x = np.zeros(n) if x0 is None else np.array(x0, float)
    scale = 1.0 + np.abs(b)
    if m and np.any(A @ x - b > 1e-9 * scale):
        return ASResult(x, np.zeros(m), np.zeros(m, bool), 0, 3)
    W: list[int] = [i for i in range(m) if abs(A[i] @ x - b[i]) <= 1e-12 * scale[i]]
    # keep W linearly independent
    Wi: list[int] = []
    for i in W:
        if np.linalg.matrix_rank(A[Wi + [i]]) == len(Wi) + 1:
            Wi.append(i)
    W = Wi
    lam_full = np.zeros(m)
    # x minimises the QP on the working set W (taken as equalities): true after
    # a full step (N&W 16.3: the next p is 0 in exact arithmetic).  Testing
    # the recomputed p against a tolerance instead made the method step by
    # rounding noise forever at some vertices with |W| = n (p ~ 1e-10 from
    # slacks of ~1e-11: 2/256 QPs at n = 16 and 13/256 at n = 32 of the tests'
    # vertex family, VERDICT r05 Weak 1).
    at_min = False
    # Bland's rule once a step was degenerate (alpha = 0): the DROP takes the
    # lowest constraint index among the negative multipliers and the blocking
    # test the lowest index among the tied ratios, so the working sets of a
    # degenerate vertex are never revisited; otherwise the most negative
    # multiplier and the first minimal ratio (N&W 16.3).
    bland = False
    for it in range(max_iter):
        g = H @ x + f
        p, lam = _eqp(H, g, A[W] if W else np.zeros((0, n)))
        if at_min or np.linalg.norm(p, np.inf) <= tol * (1.0 + np.linalg.norm(x, np.inf)):
            at_min = False
            if len(W) == 0 or lam.min() >= -tol * (1.0 + np.abs(lam).max()):
                lam_full[:] = 0
                lam_full[W] = np.maximum(lam, 0.0)
                act = np.zeros(m, bool)
                act[W] = True
                return ASResult(x, lam_full, act, it, 0)
            if bland:
                neg = [k for k in range(len(W)) if lam[k] < -tol * (1.0 + np.abs(lam).max())]
                j = min(neg, key=lambda k: W[k])
            else:
                j = int(np.argmin(lam))
            W.pop(j)
            continue
        Ap = A @ p if m else np.zeros(0)
        alpha, block = 1.0, -1
        for i in range(m):
            if i in W or Ap[i] <= 1e-14 * np.linalg.norm(A[i]) * np.linalg.norm(p):
                continue
            ai = max((b[i] - A[i] @ x) / Ap[i], 0.0)
            if ai < alpha:  # ties keep the lowest index (rows are scanned in order)
                alpha, block = ai, i
        x = x + alpha * p
        if block >= 0:
            W.append(block)
            bland = bland or alpha == 0.0
        else:
            at_min = True
    act = np.zeros(m, bool)
    act[W] = True
    return ASResult(x, lam_full, act, max_iter, 1)


def kkt_residuals(H, f, A, b, x, lam):
    """Batched KKT certificate for A x <= b.  Shapes (B,n,n),(B,n),(B,m,n),(B,m),
    (B,n),(B,m).  Returns dict of per-QP relative residuals:
      stat  ||H x + f + A^T lam||_inf / (1 + ||f||_inf + ||H||_inf ||x||_inf)
      prim  max(0, max_i (a_i x - b_i)) / (1 + ||b||_inf + ||A||_inf ||x||_inf)
      dual  max(0, -min lam) / (1 + ||lam||_inf)
      comp  max_i |lam_i (b_i - a_i x)| / ((1 + ||lam||_inf)(1 + ||b|| + ||A|| ||x||))
    """
    H, f, A, b, x, lam = (np.asarray(v, float) for v in (H, f, A, b, x, lam))
    r = np.einsum("bij,bj->bi", H, x) + f + np.einsum("bij,bi->bj", A, lam)
    xn = np.abs(x).max(axis=1)
    Hn = np.abs(H).sum(axis=2).max(axis=1)
    stat = np.abs(r).max(axis=1) / (1.0 + np.abs(f).max(axis=1) + Hn * xn)
    if A.shape[1] == 0:
        z = np.zeros(len(x))
        return {"stat": stat, "prim": z, "dual": z, "comp": z}
    An = np.abs(A).sum(axis=2).max(axis=1)
    sc = 1.0 + np.abs(b).max(axis=1) + An * xn
    slack = b - np.einsum("bij,bj->bi", A, x)
    prim = np.maximum(0.0, -slack.min(axis=1)) / sc
    ln = 1.0 + np.abs(lam).max(axis=1)
    dual = np.maximum(0.0, -lam.min(axis=1)) / ln
    comp = np.abs(lam * slack).max(axis=1) / (ln * sc)
    return {"stat": stat, "prim": prim, "dual": dual, "comp": comp}


# --------------------------------------------------------------------------
# synthetic families; numpy RNG, seeded
# --------------------------------------------------------------------------


def family_conditioned(seed: int, count: int, n: int, m: int | None = None, box: float = 25.0,
                       shift: float = 1.0, kind: str = "box"):
    """H = B^T B / (1e3 n) + shift*I  (the reference generator's P, matrix_ops.c:699-734,
    shifted so cond(H) stays <~1e6), f ~ U[-1e3, 1e3] (config.h:19-20).

    kind="box"  : A = [I; -I], b = [ub; -lb], ub = -lb = box   (m = 2n; ADMM's box,
                  qp_solvers.c:277-280, written as a dense A)
    kind="dense": A rows ~ N(0,1) normalised, b ~ U(0.1, 1) * box * ||row||... (x=0
                  strictly feasible).
    """
    rs = np.random.default_rng(seed)
    Bm = rs.uniform(-1e3, 1e3, size=(count, n, n))
    H = np.einsum("bki,bkj->bij", Bm, Bm) / (1e3 * n) + shift * np.eye(n)
    f = rs.uniform(-1e3, 1e3, size=(count, n))
    if kind == "box":
        m = 2 * n
        A = np.concatenate([np.broadcast_to(np.eye(n), (count, n, n)),
                            np.broadcast_to(-np.eye(n), (count, n, n))], axis=1).copy()
        b = np.full((count, m), float(box))
    elif kind == "dense":
        m = m or 2 * n
        A = rs.standard_normal((count, m, n))
        A /= np.linalg.norm(A, axis=2, keepdims=True)
        b = rs.uniform(0.1, 1.0, size=(count, m)) * box
    else:
        raise ValueError(kind)
    return H, f, A, b


def family_shifted(seed: int, count: int, n: int, m: int):
    """family_conditioned's dense H, f, A (box = 10) with the feasible region
    moved off the origin: xc ~ U(-20, 20)^n, b = A xc + U(0.1, 1) * 10.  xc is
    strictly feasible (slack >= 1 on every row), x = 0 in general is not, and
    about 30 % of the entries of b are negative.  Returns (H, f, A, b, xc); xc
    is the feasible x0 that active_set_solve needs."""
    H, f, A, _ = family_conditioned(seed, count, n, m=m, box=10.0, kind="dense")
    rs = np.random.default_rng([seed, 0x5F1F7])
    xc = rs.uniform(-20.0, 20.0, size=(count, n))
    b = np.einsum("bij,bj->bi", A, xc) + rs.uniform(0.1, 1.0, size=(count, m)) * 10.0
    return H, f, A, b, xc


def family_farkas(seed: int, count: int, n: int, m: int, k: int, delta: float = 1.0):
    """family_shifted with row m-1 replaced by -sum_{i<k} y_i a_i / nr
    (y ~ U(0.5, 1.5)^k, nr the norm of the sum; k <= m - 1), then the rows
    permuted per QP.  Two right-hand sides that differ in that row only:

      b_inf   (-sum y_i b_i - delta) / nr: infeasible, the multipliers (y, nr)
              are a Farkas certificate (A^T c = 0, c >= 0, b^T c = -delta < 0)
      b_feas  (-sum y_i b_i + sum y_i s_i + delta) / nr with s = b - A xc: the
              same linearly dependent rows, xc strictly feasible (slack
              delta / nr on the new row)

    Returns (H, f, A, b_inf, b_feas, xc, cert), cert (count, m) in the permuted
    row order."""
    if not 1 <= k <= m - 1:
        raise ValueError("family_farkas: 1 <= k <= m - 1")
    H, f, A, b, xc = family_shifted(seed, count, n, m)
    rs = np.random.default_rng([seed, 0xFA2CA5, k])
    y = rs.uniform(0.5, 1.5, size=(count, k))
    row = -np.einsum("bi,bij->bj", y, A[:, :k])
    nr = np.linalg.norm(row, axis=1)
    A[:, m - 1] = row / nr[:, None]
    yb = np.einsum("bi,bi->b", y, b[:, :k])
    ys = np.einsum("bi,bi->b", y, b[:, :k] - np.einsum("bij,bj->bi", A[:, :k], xc))
    b_inf, b_feas = b.copy(), b.copy()
    b_inf[:, m - 1] = (-yb - delta) / nr
    b_feas[:, m - 1] = (-yb + ys + delta) / nr
    cert = np.zeros((count, m))
    cert[:, :k] = y
    cert[:, m - 1] = nr
    for i in range(count):
        perm = rs.permutation(m)
        A[i], b_inf[i], b_feas[i], cert[i] = A[i, perm], b_inf[i, perm], b_feas[i, perm], cert[i, perm]
    return H, f, A, b_inf, b_feas, xc, cert


# --------------------------------------------------------------------------
# on-device generators (csrc/qpb_gen.hip), restated for the parity tests
# --------------------------------------------------------------------------

_M32 = 0xFFFFFFFF
_GDEG = 31


def _glibc_base(seed: int) -> list:
    """srandom_r's window s[j] = r[3 + j] (GlibcRand.seed without the discards)."""
    word = seed & _M32
    if word >= 0x80000000:
        word -= 0x100000000
    if word == 0:
        word = 1
    r = [word]
    for _ in range(1, 31):
        hi = int(word / 127773)  # C truncation
        lo = word - hi * 127773
        word = 16807 * lo - 2836 * hi
        if word < 0:
            word += 2147483647
        r.append(word)
    r += r[0:3]
    return [x & _M32 for x in r[3:34]]


def _poly_sqr(c: list) -> list:
    p = [0] * (2 * _GDEG - 1)
    for i in range(_GDEG):
        ci = c[i]
        if ci:
            for j in range(_GDEG):
                p[i + j] = (p[i + j] + ci * c[j]) & _M32
    for d in range(2 * _GDEG - 2, _GDEG - 1, -1):  # x^31 = x^28 + 1
        p[d - 3] = (p[d - 3] + p[d]) & _M32
        p[d - _GDEG] = (p[d - _GDEG] + p[d]) & _M32
    return p[:_GDEG]


def _poly_mulx(c: list) -> list:
    top = c[-1]
    c = [top] + c[:-1]
    c[_GDEG - 3] = (c[_GDEG - 3] + top) & _M32
    return c


def glibc_draws_at(seed: int, first: int, count: int) -> np.ndarray:
    """rand() outputs first .. first+count-1 after srand(seed), by jump-ahead:
    the window obeys s[t] = s[t-31] + s[t-3] (mod 2^32), output o is
    s[341 + o] >> 1, and s[T] = sum c_j s[j] with x^T mod (x^31 - x^28 - 1)
    -- the algorithm of qpb_gen.hip's ref_draws_kernel."""
    base = _glibc_base(seed)
    T0 = 310 + first
    c = [1] + [0] * (_GDEG - 1)
    for bit in range(T0.bit_length() - 1, -1, -1):
        c = _poly_sqr(c)
        if (T0 >> bit) & 1:
            c = _poly_mulx(c)
    w = []
    for _ in range(_GDEG):
        w.append(sum(ci * bi for ci, bi in zip(c, base)) & _M32)
        c = _poly_mulx(c)
    out = []
    while len(out) < count:
        for i in range(_GDEG):
            w[i] = (w[i] + w[(i + _GDEG - 3) % _GDEG]) & _M32
            if len(out) < count:
                out.append(w[i] >> 1)
    return np.array(out, dtype=np.float64)


def ref_generate_at(seed: int, index: int, n: int, prange=(-1e3, 1e3), qrange=(-1e3, 1e3), xrange=(-1e3, 1e3)):
    """QP `index` of ref_generate(seed, ...) without drawing its predecessors."""
    D = n * n + 2 * n
    r = glibc_draws_at(seed, index * D, D)

    def rn(vals, lo, hi):
        return lo + (vals * (hi - lo)) / RAND_MAX

    B = rn(r[:n * n], *prange).reshape(n, n)
    acc = np.zeros((n, n))
    for k in range(n):
        acc = acc + np.outer(B[k, :], B[k, :])
    P = acc * (1.0 / float(prange[1] * n))
    return P, rn(r[n * n:n * n + n], *qrange), rn(r[n * n + n:], *xrange)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al. 2011) on uint32 numpy arrays / ints."""
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) for v in (c0, c1, c2, c3))
    k0 = np.asarray(k0, dtype=np.uint64)
    k1 = np.asarray(k1, dtype=np.uint64)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        c1 = p1 & np.uint64(_M32)
        c3 = p0 & np.uint64(_M32)
        c0 = n0 & np.uint64(_M32)
        c2 = n2 & np.uint64(_M32)
        k0 = (k0 + np.uint64(0x9E3779B9)) & np.uint64(_M32)
        k1 = (k1 + np.uint64(0xBB67AE85)) & np.uint64(_M32)
    return c0, c1, c2, c3


def philox_uniform(seed: int, g, purpose: int, e) -> np.ndarray:
    """Element e of stream `purpose` of QP g in [0, 1) (qpb_gen.hip uniform())."""
    g = np.asarray(g, dtype=np.uint64)
    e = np.asarray(e, dtype=np.uint64)
    g, e = np.broadcast_arrays(g, e)
    c0, c1, c2, c3 = philox4x32_10(e >> np.uint64(1), g & np.uint64(_M32), g >> np.uint64(32),
                                   np.full(e.shape, purpose, dtype=np.uint64), seed & _M32, (seed >> 32) & _M32)
    odd = (e & np.uint64(1)).astype(bool)
    hi = np.where(odd, c2, c0)
    lo = np.where(odd, c3, c1)
    return ((hi >> np.uint64(5)).astype(np.float64) * 67108864.0 + (lo >> np.uint64(6)).astype(np.float64)) \
        * (1.0 / 9007199254740992.0)


def family_generate(n: int, batch: int, seed: int, family: str = "box", m: int | None = None, first: int = 0,
                    shift: float = 1.0, box: float = 10.0):
    """The qpb_generate benchmark families (H by numpy matmul: equal to the
    matrix-core product up to summation order)."""
    m = 2 * n if m is None else m
    g = np.arange(first, first + batch, dtype=np.uint64)[:, None]
    B = (-1e3 + 2e3 * philox_uniform(seed, g, 0, np.arange(n * n)[None, :])).reshape(batch, n, n)
    H = np.einsum("bki,bkj->bij", B, B) / (1e3 * n) + shift * np.eye(n)
    f = -1e3 + 2e3 * philox_uniform(seed, g, 1, np.arange(n)[None, :])
    if family == "box":
        A = np.broadcast_to(np.concatenate([np.eye(n), -np.eye(n)]), (batch, 2 * n, n)).copy()
        b = np.full((batch, 2 * n), box)
    else:
        e = np.arange(m * n)[None, :]
        u1 = philox_uniform(seed, g, 2, 2 * e)
        u2 = philox_uniform(seed, g, 2, 2 * e + 1)
        z = (np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(6.283185307179586 * u2)).reshape(batch, m, n)
        A = z * (1.0 / np.sqrt((z * z).sum(axis=2, keepdims=True)))
        b = (0.1 + 0.9 * philox_uniform(seed, g, 3, np.arange(m)[None, :])) * box
    return H, f, A, b
