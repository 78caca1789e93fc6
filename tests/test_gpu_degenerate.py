"""Degenerate QPs on every kernel route: linearly dependent rows through the
optimum, weakly active rows (a x* = b with a zero multiplier), a vertex with
more than n tight rows, exact ties in the selection key, and for
qpb_solve_box a pinned variable (lb_j == ub_j).  The other GPU parity tests
draw non-degenerate families and compare active sets bit for bit; here the
active set is not unique, so the checks are the ones that are:

  status OK, iters <= 4 (n + m) + 8, on every QP (none is excused)
  x within 1e-9 relative of the planted x* (tests/planted.py: integer data,
    exact; x* is unique because H is SPD; cond(H) < 12)
  the KKT certificate of the GPU's own answer <= 1e-9 on all four residuals
  lam >= 0 on the inequality rows, lam == 0 outside the mask
  mask within the tight rows: no slack row is ever reported active
  every row with lam* > 0 in the mask where the multipliers are unique
    (rank(A[tight]) == number of tight rows); for `dup` at least one row of
    each triple, and A^T lam == A^T lam* within 1e-9
  `ties` (not degenerate): mask bit-exact, lam within 1e-9

The reference is the planted solution, not oracle.active_set_solve, which can
hit its iteration cap at these vertices (tests/test_planted.py).  QP i of a
launch has kind i mod 3 with its own seed, so a degenerate QP's partners in the
four-per-wavefront kernels differ from it.  Each test prints and asserts > 0
the number of its QPs that really were degenerate (tight rows beyond the set
bits).
"""
import numpy as np
import pytest

import eq_oracle as EO
import planted as P

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

X_TOL = 1e-9
KKT_TOL = 1e-9
OK = 0

dense_routes = pytest.mark.parametrize("route", P.DEGENERATE, ids=[r[0] for r in P.DEGENERATE])
eq_routes = pytest.mark.parametrize("n,m,meq,B", P.EQ)
box_routes = pytest.mark.parametrize("n,B", P.BOX)


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    return q


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda() for a in arrays]


def _host(sol):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in sol]


def _relx(x, xr):
    return np.abs(x - xr).max(axis=1) / np.maximum(1.0, np.abs(xr).max(axis=1))


def _kkt(q, meq, x, lam):
    import oracle as O
    res = EO.kkt_mixed(q.H, q.f, q.A, q.b, meq, x, lam) if meq else O.kkt_residuals(q.H, q.f, q.A, q.b, x, lam)
    return {k: float(v.max()) for k, v in res.items()}


def _check(qpb, q, kinds, sol, what, meq=0, expect_degenerate=True):
    """The module docstring's assertions on one launch; q is a planted.Planted
    or PlantedBox batch (the box's fields A, b, lam, tight are the [I; -I] form's)."""
    x, lam, act, st, it = sol
    B, m, n = q.A.shape
    mask = qpb.active_mask_to_bool(act, m)
    ex = _relx(x, q.x)
    worst = _kkt(q, meq, x, lam) if (st == OK).all() else {}
    degenerate = int((q.tight.sum(axis=1) > mask.sum(axis=1)).sum())
    print(f"{what}: status {np.bincount(st, minlength=5).tolist()} x err {ex.max():.2e} "
          f"kkt {max(worst.values(), default=np.nan):.2e} iters {it.min()}..{it.max()} "
          f"degenerate {degenerate}/{B} set bits {mask.sum(axis=1).min()}..{mask.sum(axis=1).max()} "
          f"tight {q.tight.sum(axis=1).min()}..{q.tight.sum(axis=1).max()}")
    assert (st == OK).all(), (what, st, it)
    assert (it <= 4 * (n + m) + 8).all() and (it >= 1).all(), (what, it)
    assert ex.max() <= X_TOL, (what, ex)
    assert all(v <= KKT_TOL for v in worst.values()), (what, worst)
    assert (lam[:, meq:] >= 0).all(), (what, lam[:, meq:].min())
    assert (lam[~mask] == 0).all(), what
    assert not (mask & ~q.tight).any(), (what, np.nonzero((mask & ~q.tight).any(axis=1)))
    atl = np.einsum("bij,bi->bj", q.A, lam)
    atr = np.einsum("bij,bi->bj", q.A, q.lam)
    assert (_relx(atl, atr) <= X_TOL).all(), (what, _relx(atl, atr))
    for i, kind in enumerate(kinds):
        need = q.lam[i] != 0 if meq == 0 else np.concatenate([np.zeros(meq, bool), q.lam[i, meq:] > 0])
        if kind == "dup":
            for g in range(int(q.group[i].max()) + 1):
                assert mask[i, q.group[i] == g].any(), (what, i, "no row of triple", g)
        elif np.linalg.matrix_rank(q.A[i][q.tight[i]]) == q.tight[i].sum():
            assert mask[i, need].all(), (what, i, kind, np.nonzero(need & ~mask[i]))
            assert np.abs(lam[i] - q.lam[i]).max() <= X_TOL * (1.0 + np.abs(q.lam[i]).max()), (what, i, kind)
    if meq:
        assert mask[:, :meq].all(), what
    if expect_degenerate:
        assert degenerate > 0, what
    return mask


# ---------------------------------------------------------------- qpb_solve
@dense_routes
def test_degenerate_dense(qpb, route):
    """weak / dup / vertex interleaved on every dense route (gi_dense's four
    forms, gi_wave, gi_mixed, gi_gram up to its full tile set).  On gi_mixed a
    degenerate fp32 active set must verify or fall back to the fp64 re-solve:
    the bars are the same."""
    name, n, m, B, flags = route
    q, kinds = P.dense_batch(n, m, B)
    sol = _host(qpb.solve(*_dev(q.H, q.f, q.A, q.b), flags=flags))
    _check(qpb, q, kinds, sol, name)


@dense_routes
def test_ties_dense(qpb, route):
    """Exact ties in the selection key: every upper row violated by the same
    amount with the same norm.  The solution is not degenerate: mask bit-exact
    (the n upper rows), lam = 2 within 1e-9.  Three copies, so that the
    four-per-wavefront kernel holds more than one."""
    name, n, m, B, flags = route
    q, kinds = P.batch_of(lambda s, k: P.planted_dense(n, m, s, k), min(B, 3), ("ties",), 0)
    sol = _host(qpb.solve(*_dev(q.H, q.f, q.A, q.b), flags=flags))
    mask = _check(qpb, q, kinds, sol, name + " ties", expect_degenerate=False)
    assert np.array_equal(mask, q.tight), name
    assert np.abs(sol[1] - q.lam).max() <= 2.0 * X_TOL


# ------------------------------------------------------------- qpb_solve_eq
@eq_routes
def test_degenerate_eq(qpb, n, m, meq, B):
    """weak / dup on the inequality rows beside meq equalities with
    multipliers of both signs (the EQ forms of gi_dense and gi_wave); the
    certificate is eq_oracle.kkt_mixed and every equality bit is set."""
    q, kinds = P.eq_batch(n, m, meq, B)
    sol = _host(qpb.solve_eq(*_dev(q.H, q.f, q.A, q.b), meq))
    _check(qpb, q, kinds, sol, f"eq ({n},{m},{meq})", meq=meq)
    assert (np.abs(sol[1][:, :meq] - q.lam[:, :meq]).max(axis=1) <= X_TOL * (1.0 + np.abs(q.lam).max(axis=1))).all()


# ------------------------------------------------------------ qpb_solve_box
def _box_and_dense(qpb, q):
    box = _host(qpb.solve_box(*_dev(q.H, q.f, q.lb, q.ub)))
    dense = _host(qpb.solve(*_dev(q.H, q.f, q.A, q.b)))
    return box, dense


@box_routes
def test_degenerate_box(qpb, n, B):
    """weak / pinned / all_pinned interleaved through qpb_solve_box (gi_box
    padded and full, gi_wave's and gi_gram's BOX forms) and through qpb_solve
    on the explicit [I; -I] form of the same QPs: both meet the bars, with the
    same statuses, x within 1e-9 of each other and the same bits on every
    variable whose bits are determined (neither pinned nor weakly active).  A
    pinned variable (rows e_j and -e_j both tight, dependent) ends on its
    bound with lam_ub[j] - lam_lb[j] = mu_j within 1e-9."""
    q, kinds = P.box_batch(n, B)
    box, dense = _box_and_dense(qpb, q)
    mb = _check(qpb, q, kinds, box, f"box n={n}")
    md = _check(qpb, q, kinds, dense, f"box n={n} as [I; -I]")
    assert np.array_equal(box[3], dense[3])
    assert _relx(box[0], dense[0]).max() <= X_TOL
    plain = np.concatenate([q.plain, q.plain], axis=1)
    assert np.array_equal(mb[plain], md[plain]) and np.array_equal(mb[plain], q.tight[plain])
    for what, (x, lam, _, _, _) in (("box", box), ("dense", dense)):
        assert (np.abs(x - q.lb)[q.pinned] <= X_TOL * np.maximum(1.0, np.abs(q.lb[q.pinned]))).all(), what
        mu = lam[:, :n] - lam[:, n:]
        err = np.abs(mu - q.mu).max(axis=1) / (1.0 + np.abs(q.mu).max(axis=1))
        print(f"{what} n={n}: mu err {err.max():.2e} pinned {int(q.pinned.sum())} "
              f"mu<0 {int((q.mu[q.pinned] < 0).sum())} mu>0 {int((q.mu[q.pinned] > 0).sum())}")
        assert err.max() <= X_TOL, (what, err)


@box_routes
def test_ties_box(qpb, n, B):
    """planted_box's ties (the unit box, every upper bound violated alike)
    through both entry points: mask bit-exact and equal, lam = 2 within 1e-9."""
    q, kinds = P.batch_of(lambda s, k: P.planted_box(n, s, k), min(B, 3), ("ties",), 0)
    box, dense = _box_and_dense(qpb, q)
    for what, sol in (("box", box), ("[I; -I]", dense)):
        mask = _check(qpb, q, kinds, sol, f"{what} n={n} ties", expect_degenerate=False)
        assert np.array_equal(mask, q.tight), what
        assert np.abs(sol[1] - q.lam).max() <= 2.0 * X_TOL
    assert np.array_equal(box[2], dense[2])
