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
import range_box_oracle as BO
import range_oracle as RO
import range_planted_checks as C


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


# ---------------------------------------------------------- range families
def _range_claims(q, kinds, meq, what, thin_from=None):
    """What every planted range batch claims: the certificate is exactly 0,
    `side` is what the bounds say, lam* has the sign its side names, H is
    well conditioned, slack rows keep 1 on both sides and a tight row's other
    bound is 1 away or more (THIN for `thin`, and on the rows >= thin_from:
    the variable bounds of a range-box QP)."""
    _zero_kkt(RO.kkt_range(q.H, q.f, q.A, q.bl, q.bu, meq, q.x, q.lam), what)
    ax = np.einsum("bij,bj->bi", q.A, q.x)
    at_u, at_l = ax == q.bu, ax == q.bl
    assert np.array_equal(q.side == 2, at_u & at_l) and np.array_equal(q.side == 1, at_u & ~at_l)
    assert np.array_equal(q.side == -1, at_l & ~at_u) and np.array_equal(q.side == 0, ~at_u & ~at_l)
    assert (q.side[:, :meq] == 2).all() and (q.lam[:, :meq] != 0).all()
    assert (q.bl <= ax).all() and (ax <= q.bu).all()
    wide = np.abs(q.side) == 1
    assert (q.lam[q.side == 0] == 0).all()
    assert (np.sign(q.lam[wide & (q.lam != 0)]) == q.side[wide & (q.lam != 0)]).all()
    assert np.linalg.cond(q.H).max() < 12.0
    for i, kind in enumerate(kinds):
        other = np.minimum(q.bu[i] - ax[i], ax[i] - q.bl[i])[q.side[i] == 0]
        assert (other >= 1.0).all(), (what, i)
        width = q.bu[i] - q.bl[i]
        start = 0 if kind == "thin" else len(width) if thin_from is None else thin_from
        narrow = wide[i] & (np.arange(len(width)) >= start)
        assert (width[narrow] == P.THIN).all() and (width[wide[i] & ~narrow] >= 1.0).all(), (what, i, kind)


def _range_kind_claims(q, kinds, n, meq, nf, mi, rows):
    """The counts and ranks of each kind on the rows `rows` (a slice: the G
    rows beyond the equalities); nf: columns left to them."""
    for i, kind in enumerate(kinds):
        side, lam, group = q.side[i, rows], q.lam[i, rows], q.group[i, rows]
        nt, nz = int((side != 0).sum()), int((lam != 0).sum())
        tight_all = q.side[i] != 0
        rank = np.linalg.matrix_rank(q.A[i][tight_all])
        k3 = max(1, min(nf // 3, mi // 3))
        if kind == "weak":
            assert (nt, nz) == (2 * k3, k3) and (np.abs(side[side != 0]) == 1).all(), (i, nt, nz)
            assert rank == tight_all.sum(), (i, rank)
        elif kind == "dup":
            k = max(1, min(nf // 2, mi // 3))
            assert (nt, nz) == (3 * k, k) and rank == tight_all.sum() - 2 * k, (i, nt, nz, rank)
            for g in range(k):
                r = np.nonzero(group == g)[0]
                assert len(r) == 3 and (lam[r] != 0).sum() == 1
                a, bl, bu, s = q.A[i, rows][r], q.bl[i, rows][r], q.bu[i, rows][r], side[r]
                base = int(np.nonzero(lam[r] != 0)[0][0])
                rest = [j for j in range(3) if j != base]
                col = np.nonzero(a[base])[0][0]
                assert sorted(float(a[j][col] / a[base][col]) for j in rest) == [-1.0, 2.0]
                for j in rest:
                    c = a[j][col] / a[base][col]
                    assert np.array_equal(a[j], c * a[base])
                    if c < 0:  # the same half-space in the other orientation, tight on the opposite side
                        assert s[j] == -s[base] and bl[j] == -bu[base] and bu[j] == -bl[base]
                    else:
                        assert s[j] == s[base] and bl[j] == 2 * bl[base] and bu[j] == 2 * bu[base]
        elif kind == "vertex":
            p = max(1, nf // 2)
            assert (nt, nz) == (min(mi, nf + p), p) and (np.abs(side[side != 0]) == 1).all(), (i, nt, nz)
            assert rank == min(tight_all.sum(), n), (i, rank)
        elif kind == "pinned":
            assert (nt, nz) == (2 * k3, k3) and (side[side != 0] == 2).all(), (i, nt, nz)
            assert rank == tight_all.sum() - k3, (i, rank)
            for g in range(k3):
                r = np.nonzero(group == g)[0]
                assert len(r) == 2 and (lam[r] != 0).sum() == 1
                assert np.array_equal(q.A[i, rows][r[0]], q.A[i, rows][r[1]])
        elif kind == "thin":
            k = max(1, min(nf // 2, mi // 2))
            assert (nt, nz) == (k, k) and rank == tight_all.sum(), (i, nt, nz, rank)
        if kind not in ("dup", "pinned", "dup_bound"):
            assert (group == -1).all()


@pytest.mark.parametrize("n,m,meq,B", P.RANGE)
def test_planted_range(n, m, meq, B):
    """The interleaved degenerate batch and the three `thin` QPs of every RANGE
    route, as tests/test_gpu_range_degenerate.py launches them."""
    nf, mi = n - meq, m - meq
    rows = slice(meq, m)
    q, kinds = P.range_batch(n, m, meq, B)
    t, tk = P.range_batch(n, m, meq, 3, kinds=("thin",))
    for b, ks in ((q, kinds), (t, tk)):
        _range_claims(b, ks, meq, (n, m, meq))
        _range_kind_claims(b, ks, n, meq, nf, mi, rows)
        assert (b.group[:, :meq] == -1).all()
    assert set(kinds) == set(P.RANGE_KINDS)
    # multipliers of both signs, zero-width rows loaded from either side
    lam = q.lam[:, meq:]
    assert (lam[q.side[:, meq:] == 2] > 0).any() and (lam[q.side[:, meq:] == 2] < 0).any()
    assert (q.side == 1).any() and (q.side == -1).any()
    # every QP of the degenerate batch is degenerate: tight rows beyond the loaded ones
    assert ((q.side != 0).sum(axis=1) > (q.lam != 0).sum(axis=1)).all()
    assert ((t.side != 0).sum(axis=1) == (t.lam != 0).sum(axis=1)).all()
    # rows are permuted: tight rows land in the last word too at m > 32
    assert (q.side[:, -min(mi, 8):] != 0).any()
    # the rows that must reach a flip: tight on the side opposite to the one violated at x0 = -H^-1 f
    opp = P.opposite_side_rows(q, meq)
    per_kind = {k: int(opp[[i for i, kk in enumerate(kinds) if kk == k]].sum()) for k in P.RANGE_KINDS}
    thin_opp = int(P.opposite_side_rows(t, meq).sum())
    print(f"({n},{m},{meq}): opposite-side rows {per_kind} thin {thin_opp}")
    assert per_kind["weak"] > 0 and per_kind["vertex"] > 0 and thin_opp > 0
    # the first six QPs alone (test_degenerate_range_factored_one_qp_at_a_time) have such rows too
    first = {k: int(opp[[i for i in range(6) if kinds[i] == k]].sum()) for k in ("weak", "vertex")}
    assert first["weak"] > 0 and first["vertex"] > 0, first
    # vertex: degeneracy is a property of the input.  More tight rows than n - meq wherever the shape has
    # that many (m > n); at m - meq == n - meq every row is tight and half of them carry no multiplier.
    for i, kind in enumerate(kinds):
        if kind == "vertex":
            nt = int((q.side[i, meq:] != 0).sum())
            assert nt > nf if mi > nf else (nt == mi and nt > (q.lam[i, meq:] != 0).sum()), (i, nt)


@pytest.mark.parametrize("n,m,meq,B", P.RANGE_SHARED)
def test_planted_range_shared(n, m, meq, B):
    q, kinds = P.range_shared_batch(n, m, meq, B)
    assert (q.H == q.H[0]).all() and (q.A == q.A[0]).all()
    assert set(kinds) == set(P.RANGE_SHARED_KINDS)
    _range_claims(q, kinds, meq, ("shared", n, m, meq))
    _range_kind_claims(q, kinds, n, meq, n - meq, m - meq, slice(meq, m))
    # every QP its own x*, tight set and sides
    assert len({tuple(v) for v in q.x}) == B and len({tuple(v) for v in q.side}) == B
    opp = P.opposite_side_rows(q, meq)
    per_kind = {k: int(opp[[i for i, kk in enumerate(kinds) if kk == k]].sum()) for k in P.RANGE_SHARED_KINDS}
    print(f"shared ({n},{m},{meq}): opposite-side rows {per_kind}")
    assert all(v > 0 for v in per_kind.values())
    for i, kind in enumerate(kinds):
        if kind == "vertex":
            assert (q.side[i, meq:] != 0).sum() > n - meq


@pytest.mark.parametrize("n,mg,meq,B", P.RANGE_BOX)
def test_planted_range_box(n, mg, meq, B):
    b, kinds = P.range_box_batch(n, mg, meq, B)
    q = P.PlantedRange(b.H, b.f, b.A, b.lo, b.hi, b.x, b.lam, b.side, b.group)
    m = mg + n
    assert set(kinds) == set(P.range_box_kinds(mg, meq))
    _range_claims(q, kinds, meq, ("box", n, mg, meq), thin_from=mg)
    A, lo, hi = BO.materialise(b.G, b.bl, b.bu, b.lb, b.ub, n)
    assert np.array_equal(A, b.A) and np.array_equal(lo, b.lo) and np.array_equal(hi, b.hi)
    assert np.array_equal(b.lam, np.concatenate([b.lam_g, b.mu], axis=1))
    assert np.array_equal(b.f, -np.einsum("bij,bj->bi", b.H, b.x) - np.einsum("bij,bi->bj", b.G, b.lam_g) - b.mu)
    assert np.array_equal(b.pinned, b.lb == b.ub) and np.array_equal(b.pinned, b.side[:, mg:] == 2)
    kb = max(1, (n - meq) // 6)
    vtight = b.side[:, mg:] != 0
    for i, kind in enumerate(kinds):
        nfree = n - meq - int(vtight[i].sum())
        if kind == "dup_bound":
            kd = max(1, min(n // 4, (mg - meq) // 2))
            assert vtight[i].sum() == kb + kd and (b.mu[i] != 0).sum() == kb + kd
            for g in range(kd):
                r = np.nonzero(b.group[i] == g)[0]
                assert len(r) == 2 and r[0] < mg <= r[1]
                j = r[1] - mg
                assert b.G[i, r[0], j] in (1.0, 2.0) and np.count_nonzero(b.G[i, r[0]]) == 1
                assert b.side[i, r[0]] == b.side[i, r[1]] != 0 and b.lam[i, r[0]] == 0 and b.mu[i, j] != 0
            assert ((b.group[i] >= 0).sum(), (b.side[i, meq:mg] != 0).sum()) == (2 * kd, kd)
        else:
            assert vtight[i].sum() == (3 * kb if kind == "pinned" else 2 * kb)
            assert (b.mu[i] != 0).sum() == (2 * kb if kind == "pinned" else kb)
            assert b.pinned[i].sum() == (kb if kind == "pinned" else 0)
            if mg > meq:
                _range_kind_claims(P.PlantedRange(*(v[i:i + 1] for v in q)), [kind], n, meq, nfree, mg - meq,
                                   slice(meq, mg))
    pm = b.mu[b.pinned]
    assert (pm > 0).any() and (pm < 0).any()
    assert ((q.side != 0).sum(axis=1) > (q.lam != 0).sum(axis=1)).all()  # every QP is degenerate
    # the rows that must reach a flip (tight on the side opposite to the one violated at x0 = -H^-1 f): on every
    # route, for weak and for vertex, and among the register-made rows >= mg (all there are at mg = 0)
    x0 = -np.linalg.solve(q.H, q.f[:, :, None])[:, :, 0]
    a0 = np.einsum("bij,bj->bi", q.A, x0)
    opp = ((q.side == 1) & (a0 < q.bl)) | ((q.side == -1) & (a0 > q.bu))
    assert np.array_equal(opp[:, meq:].sum(axis=1), P.opposite_side_rows(q, meq))
    per_kind = {k: int(opp[[i for i, kk in enumerate(kinds) if kk == k]].sum()) for k in set(kinds)}
    print(f"box ({n},{mg},{meq}): opposite-side rows {per_kind}, of them variable bounds {int(opp[:, mg:].sum())}")
    assert per_kind["weak"] > 0 and per_kind["vertex"] > 0 and opp[:, mg:].sum() > 0
    for k in ("weak", "vertex"):
        assert opp[[i for i, kk in enumerate(kinds) if kk == k]][:, mg:].sum() > 0, k
    if "dup_bound" in kinds:  # e_j occurs, and 2 e_j wherever a QP has two pairs
        scale = b.G[b.group[:, :mg] >= 0].max(axis=1)
        assert (scale == 1.0).any() and ((scale == 2.0).any() or min(n // 4, (mg - meq) // 2) <= 1)


def _one_hot_range_checks(h, n, m, meq, box_rows=0):
    H, f, A, bl, bu = h.tiled()
    K = m - meq
    assert len(h.row) == 2 * K and np.array_equal(h.row, meq + np.tile(np.arange(K), 2))
    assert np.array_equal(h.lower, np.arange(2 * K) >= K)
    assert (h.lam[~h.lower] > 0).all() and np.array_equal(h.lam[h.lower], -h.lam[~h.lower])
    lam = np.zeros(bl.shape)
    lam[np.arange(2 * K), h.row] = h.lam
    lam[:, :meq] = h.lam_eq
    worst = max(float(v.max()) for v in RO.kkt_range(H, f, A, bl, bu, meq, h.x, lam).values())
    assert worst <= 1e-13, worst
    au = h.A @ h.xu
    q = np.arange(2 * K)
    viol_u, viol_l = au[None, :] - bu, bl - au[None, :]
    assert np.allclose(viol_u[q[~h.lower], h.row[~h.lower]], 1.0, atol=1e-12)
    assert np.allclose(viol_l[q[h.lower], h.row[h.lower]], 1.0, atol=1e-12)
    viol_u[q[~h.lower], h.row[~h.lower]] = -np.inf
    viol_l[q[h.lower], h.row[h.lower]] = -np.inf
    assert (np.abs(viol_u[:, :meq]) <= 1e-12).all() and (np.abs(viol_l[:, :meq]) <= 1e-12).all()
    assert (viol_u[:, meq:] <= -3.9).all() and (viol_l[:, meq:] <= -3.9).all()  # one side of one row is violated at xu
    ax = h.x @ h.A.T
    slack = np.minimum(bu - ax, ax - bl)
    slack[q, h.row] = np.maximum(bu - ax, ax - bl)[q, h.row]  # the active row's other side
    slack[:, :meq] = np.inf
    print(f"one-hot range ({n},{m},{meq}) box_rows {box_rows}: least slack {slack.min():.2f}")
    assert slack.min() > P.MIN_SLACK
    assert np.array_equal(h.A[m - box_rows:], np.eye(n)[n - box_rows:])
    assert np.allclose(np.linalg.norm(h.A, axis=1), 1.0, atol=1e-12)
    assert 1.0 < np.linalg.cond(h.H) < 10.0


@pytest.mark.parametrize("n,m,meq,B", P.RANGE)
def test_one_hot_range(n, m, meq, B):
    _one_hot_range_checks(P.one_hot_range(n, m, meq, P.seed_of(n, m) + meq), n, m, meq)


@pytest.mark.parametrize("n,mg,meq,B", P.RANGE_BOX)
def test_one_hot_range_box(n, mg, meq, B):
    m = mg + n
    _one_hot_range_checks(P.one_hot_range(n, m, meq, P.seed_of(n, m) + meq, box_rows=n), n, m, meq, box_rows=n)


# --------------------------------------------- the shared checker has teeth
def _mutations(q, meq):
    """(name, function on a planted answer) pairs: each breaks one QP."""
    B, m = q.lam.shape

    def pick(cond, what):
        idx = np.argwhere(cond)
        assert len(idx), what
        return tuple(idx[len(idx) // 2])

    act = q.lam != 0
    wide = np.abs(q.side) == 1
    ineq = np.arange(m)[None, :] >= meq

    def flip_lower(s):
        i, j = pick(act & wide & ineq, "an active row of positive width")
        low = RO.unpack_bits(s[3], m)
        low[i, j] ^= True
        s[3] = RO.pack_bits(low)

    def negate_lam(s):
        i, j = pick(act & wide & ineq, "a loaded row")
        s[1][i, j] = -s[1][i, j]

    def shift_lam(s):
        i, j = pick(act[:, :-1] & ~act[:, 1:] & ineq[:, :-1], "a loaded row with an unloaded neighbour")
        s[1][i, j + 1], s[1][i, j] = s[1][i, j], s[1][i, j + 1]

    def slack_bit(s):
        i, j = pick(q.side == 0, "a slack row")
        a = RO.unpack_bits(s[2], m)
        a[i, j] = True
        s[2] = RO.pack_bits(a)

    def move_x(s):
        i, j = pick(ineq & np.ones((B, 1), bool), "a row")
        s[0][i] += 1e-6 * q.A[i, j] / np.linalg.norm(q.A[i, j])

    return [("lower bit flipped", flip_lower), ("lam negated", negate_lam), ("lam one slot off", shift_lam),
            ("active bit on a slack row", slack_bit), ("x moved by 1e-6", move_x)]


def _teeth(q, kinds, meq, what):
    C.check(q, kinds, C.planted_answer(q, meq), what, meq)
    for name, mutate in _mutations(q, meq):
        sol = C.planted_answer(q, meq)
        mutate(sol)
        with pytest.raises(AssertionError):
            C.check(q, kinds, sol, f"{what}, {name}", meq)


@pytest.mark.parametrize("n,m,meq,B", P.RANGE)
def test_range_checker_accepts_the_planted_answer_and_rejects_each_mutation(n, m, meq, B):
    _teeth(*P.range_batch(n, m, meq, B), meq, f"({n},{m},{meq})")
    _teeth(*P.range_batch(n, m, meq, 3, kinds=("thin",)), meq, f"({n},{m},{meq}) thin")


@pytest.mark.parametrize("n,m,meq,B", P.RANGE_SHARED)
def test_range_checker_on_the_shared_batches(n, m, meq, B):
    _teeth(*P.range_shared_batch(n, m, meq, B), meq, f"shared ({n},{m},{meq})")


@pytest.mark.parametrize("n,mg,meq,B", P.RANGE_BOX)
def test_range_checker_on_the_box_batches(n, mg, meq, B):
    b, kinds = P.range_box_batch(n, mg, meq, B)
    q = P.PlantedRange(b.H, b.f, b.A, b.lo, b.hi, b.x, b.lam, b.side, b.group)
    _teeth(q, kinds, meq, f"box ({n},{mg},{meq})")
