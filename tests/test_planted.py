"""tests/planted.py checked on the CPU: what the GPU tests take as exact is
exact, and each generator's claims about its own output hold, at every
route's shape and seed (the batches here are the GPU tests' batches).

KKT residuals of the planted (x*, lam*) are asserted == 0.0, not <= eps:
all data are small integers in fp64, so every product and sum is exact.
"""
import numpy as np
import pytest

import eq_oracle as EO
import oracle as O
import planted as P


def _zero_kkt(res, what):
    worst = {k: float(v.max()) for k, v in res.items()}
    assert all(v == 0.0 for v in worst.values()), (what, worst)


def _ranks(A, tight):
    return np.array([np.linalg.matrix_rank(A[i][tight[i]]) for i in range(len(A))])


# ------------------------------------------------------------------ dense
@pytest.mark.parametrize("route", P.DEGENERATE, ids=[r[0] for r in P.DEGENERATE])
def test_planted_dense(route):
    name, n, m, B, _ = route
    q, kinds = P.dense_batch(n, m, B)
    _zero_kkt(O.kkt_residuals(q.H, q.f, q.A, q.b, q.x, q.lam), name)
    slack = q.b - np.einsum("bij,bj->bi", q.A, q.x)
    assert np.array_equal(slack == 0.0, q.tight) and (slack[~q.tight] >= 1.0).all()
    assert (q.lam >= 0).all() and (q.lam[~q.tight] == 0).all()
    assert np.abs(np.linalg.eigvalsh(q.H)).min() >= n - 1e-9 and np.linalg.cond(q.H).max() < 12.0
    rank = _ranks(q.A, q.tight)
    for i, kind in enumerate(kinds):
        nt, pos = int(q.tight[i].sum()), int((q.lam[i] > 0).sum())
        if kind == "weak":
            k = max(1, min(n // 3, m // 3))
            assert (nt, pos, rank[i]) == (2 * k, k, 2 * k), (i, nt, pos, rank[i])
            assert (q.group[i] == -1).all()
        elif kind == "dup":
            k = max(1, min(n // 2, m // 3))
            assert (nt, pos, rank[i]) == (3 * k, k, k), (i, nt, pos, rank[i])
            for g in range(k):
                rows = np.nonzero(q.group[i] == g)[0]
                assert len(rows) == 3 and q.tight[i, rows].all()
                assert (q.lam[i, rows] > 0).sum() == 1
                a, bb = q.A[i, rows], q.b[i, rows]
                base = rows[np.argmin(np.abs(a).sum(axis=1))]
                ratio = sorted(float(np.abs(a[j]).sum() / np.abs(q.A[i, base]).sum()) for j in range(3))
                assert ratio == [1.0, 1.0, 2.0], ratio
                for j in range(3):
                    s = np.abs(a[j]).sum() / np.abs(q.A[i, base]).sum()
                    assert np.array_equal(a[j], s * q.A[i, base]) and bb[j] == s * q.b[i, base]
            assert (q.group[i] >= 0).sum() == 3 * k
        else:
            assert kind == "vertex"
            assert nt == min(m, n + max(1, n // 2)) and pos == max(1, n // 2)
            assert rank[i] == min(nt, n), (i, rank[i])
    # every QP is degenerate: tight rows beyond the strictly active ones
    assert (q.tight.sum(axis=1) > (q.lam > 0).sum(axis=1)).all()
    # rows are permuted: tight rows land in the last word too at m > 32
    assert q.tight[:, -min(m, 8):].any()


@pytest.mark.parametrize("route", P.DEGENERATE, ids=[r[0] for r in P.DEGENERATE])
def test_planted_ties(route):
    name, n, m, B, _ = route
    q = P.planted_dense(n, m, 0, "ties")
    _zero_kkt(O.kkt_residuals(*(v[None] for v in (q.H, q.f, q.A, q.b, q.x, q.lam))), name)
    assert np.array_equal(q.tight, np.arange(m) < n) and np.array_equal(q.lam > 0, q.tight)
    assert np.array_equal(q.b - q.A @ q.x == 0.0, q.tight)
    xu = np.linalg.solve(q.H, -q.f)
    viol = q.A @ xu - q.b
    assert (viol[q.tight] == 2.0).all() and (viol[~q.tight] < 0).all()  # the same key on every violated row
    assert np.linalg.matrix_rank(q.A[q.tight]) == q.tight.sum()


# --------------------------------------------------------------------- eq
@pytest.mark.parametrize("n,m,meq,B", P.EQ)
def test_planted_eq(n, m, meq, B):
    q, kinds = P.eq_batch(n, m, meq, B)
    _zero_kkt(EO.kkt_mixed(q.H, q.f, q.A, q.b, meq, q.x, q.lam), (n, m, meq))
    assert q.tight[:, :meq].all() and (q.lam[:, :meq] != 0).all()
    assert (q.lam[:, :meq] < 0).any(axis=1).all() and (q.lam[:, :meq] > 0).any(axis=1).all() or meq == 1
    assert (q.lam[:, meq:] >= 0).all() and (q.lam[~q.tight] == 0).all()
    slack = q.b - np.einsum("bij,bj->bi", q.A, q.x)
    assert np.array_equal(slack == 0.0, q.tight) and (slack[~q.tight] >= 1.0).all()
    rank = _ranks(q.A, q.tight)
    for i, kind in enumerate(kinds):
        nt = int(q.tight[i, meq:].sum())
        if kind == "weak":
            k = max(1, min((n - meq) // 3, (m - meq) // 3))
            assert nt == 2 * k and rank[i] == meq + 2 * k
        else:
            k = max(1, min((n - meq) // 2, (m - meq) // 3))
            assert nt == 3 * k and rank[i] == meq + k
            assert sorted(np.bincount(q.group[i][q.group[i] >= 0]).tolist()) == [3] * k
        assert (q.group[i, :meq] == -1).all()


# -------------------------------------------------------------------- box
@pytest.mark.parametrize("n,B", P.BOX)
def test_planted_box(n, B):
    q, kinds = P.box_batch(n, B)
    _zero_kkt(O.kkt_residuals(q.H, q.f, q.A, q.b, q.x, q.lam), n)
    assert (q.lb <= q.x).all() and (q.x <= q.ub).all()
    assert np.array_equal(q.b, np.concatenate([q.ub, -q.lb], axis=1))
    slack = q.b - np.einsum("bij,bj->bi", q.A, q.x)
    assert np.array_equal(slack == 0.0, q.tight)
    assert np.array_equal(q.mu, q.lam[:, :n] - q.lam[:, n:]) and (q.lam >= 0).all()
    assert np.array_equal(q.pinned, q.lb == q.ub)
    k = max(1, n // 3)
    for i, kind in enumerate(kinds):
        both = q.tight[i, :n] & q.tight[i, n:]
        assert np.array_equal(both, q.pinned[i])
        weak = (q.tight[i, :n] | q.tight[i, n:]) & (q.mu[i] == 0) & ~q.pinned[i]
        assert np.array_equal(q.plain[i], ~(weak | q.pinned[i]))
        if kind == "weak":
            assert weak.sum() == k and not q.pinned[i].any() and (q.mu[i] != 0).sum() == k
        elif kind == "pinned":
            assert q.pinned[i].sum() == k and (q.mu[i][q.pinned[i]] != 0).all() and not weak.any()
        else:
            assert q.pinned[i].all() and np.array_equal(q.x[i], q.lb[i])
    pm = q.mu[q.pinned]
    assert (pm > 0).any() and (pm < 0).any()
    assert (q.tight.sum(axis=1) > (q.lam > 0).sum(axis=1)).all()
    t = P.planted_box(n, 0, "ties")
    _zero_kkt(O.kkt_residuals(*(v[None] for v in (t.H, t.f, t.A, t.b, t.x, t.lam))), ("ties", n))
    assert np.array_equal(t.tight, np.arange(2 * n) < n)


# ---------------------------------------------------------------- one-hot
def _one_hot_checks(h, meq=0, lam_eq=None):
    """The closed form is a KKT point whose active set is its one row (the
    helper asserted the slack of the others itself)."""
    H, f, A, b = h.tiled()
    lam = np.zeros(b.shape)
    lam[np.arange(len(h.row)), h.row] = h.lam
    if meq:
        lam[:, :meq] = lam_eq
        res = EO.kkt_mixed(H, f, A, b, meq, h.x, lam)
    else:
        res = O.kkt_residuals(H, f, A, b, h.x, lam)
    worst = max(float(v.max()) for v in res.values())
    assert worst <= 1e-13, worst
    at_xu = b - h.xu @ h.A.T
    assert np.allclose(at_xu[np.arange(len(h.row)), h.row], -1.0, atol=1e-12)
    at_xu[np.arange(len(h.row)), h.row] = np.inf
    assert (np.abs(at_xu[:, :meq]) <= 1e-12).all() and (at_xu[:, meq:] >= 3.9).all()
    assert np.array_equal(h.mask().sum(axis=1), np.ones(len(h.row)))
    assert 1.0 < np.linalg.cond(h.H) < 10.0


@pytest.mark.parametrize("route", P.ONE_HOT, ids=[r[0] for r in P.ONE_HOT])
def test_one_hot_rows(route):
    name, n, m, _, _ = route
    h = P.one_hot_rows(n, m, P.seed_of(n, m))
    assert h.b.shape == (m, m) and np.array_equal(h.row, np.arange(m))
    _one_hot_checks(h)


@pytest.mark.parametrize("n", P.ONE_HOT_BOX_N)
def test_one_hot_bounds(n):
    h, lb, ub = P.one_hot_bounds(n, P.seed_of(n, 2 * n))
    assert np.array_equal(h.b, np.concatenate([ub, -lb], axis=1)) and (lb < ub).all()
    assert np.array_equal(h.mask(), np.eye(2 * n, dtype=bool))
    _one_hot_checks(h)


@pytest.mark.parametrize("n,m,meq,B", P.EQ)
def test_one_hot_eq(n, m, meq, B):
    h, lam_eq = P.one_hot_eq(n, m, meq, P.seed_of(n, m) + meq)
    assert np.array_equal(h.row, meq + np.arange(m - meq))
    _one_hot_checks(h, meq, lam_eq)


# ------------------------------------------------- what the oracle still gets
@pytest.mark.parametrize("n,m", [(32, 64), (48, 96)])
def test_oracle_on_vertex_family(n, m):
    """A recorded fact, not a requirement on the oracle: on the `vertex`
    family (n + n/2 tight rows through x*), started at x* itself,
    oracle.active_set_solve returns x within 1e-9 of x* for every QP.  Its
    status is NOT asserted: in a probe of 240 exactly degenerate QPs it ran
    into its 500-iteration cap on 7 (3 at (32, 64), 4 at (48, 96)), all of this
    family, with x still correct.  That is why the degenerate GPU tests take
    the planted solution, not the oracle, as their reference."""
    q, _ = P.dense_batch(n, m, 6, kinds=("vertex",))
    capped = 0
    for i in range(len(q.f)):
        r = O.active_set_solve(q.H[i], q.f[i], q.A[i], q.b[i], x0=q.x[i])
        capped += r.status != 0
        assert np.abs(r.x - q.x[i]).max() / max(1.0, np.abs(q.x[i]).max()) <= 1e-9, i
    print(f"({n},{m}): oracle capped on {capped} of {len(q.f)}")
