"""Every row index as the one active row, on every kernel route.

The kernels map rows to lanes (one or two per lane in gi_dense), to wavefront
lanes (gi_wave) and to tiles (gi_gram), and write `active` in 32-bit words;
the random families of the other tests make a given row active only by
chance.  Here a launch holds one QP per row (tests/planted.py's one-hot
families: QP k violates row k alone at the unconstrained minimiser, every
other row keeps a slack above 0.5 at the closed-form solution, cond(H) < 10),
so a wrong bit for row 31, 32, 63 or 255, or a lam written one slot off in a
padded form, fails:

  status OK
  mask == the identity matrix, bit for bit
  lam[k, k] within 1e-9 relative of 1 / (a_k H^{-1} a_k), every other lam == 0.0
  x within 1e-9 relative of xu - lam_k H^{-1} a_k
  iters the same for all QPs of the launch: 2 on the fp64 routes (one row
    taken, one trip that finds nothing; tests/test_gpu_eq.py's convention),
    equality across the launch only on gi_mixed
"""
import numpy as np
import pytest

import planted as P

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

X_TOL = 1e-9
OK = 0


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


def _check(qpb, h, sol, what, iters=None, meq=0, lam_eq=None):
    x, lam, act, st, it = sol
    Q, m = h.b.shape
    mask = qpb.active_mask_to_bool(act, m)
    want = h.mask()
    want[:, :meq] = True
    k = np.arange(Q)
    ex = np.abs(x - h.x).max(axis=1) / np.maximum(1.0, np.abs(h.x).max(axis=1))
    el = np.abs(lam[k, h.row] - h.lam) / h.lam
    wrong = np.nonzero((mask != want).any(axis=1))[0]
    print(f"{what}: {Q} QPs, status {np.bincount(st, minlength=5).tolist()} x err {ex.max():.2e} "
          f"lam err {el.max():.2e} iters {it.min()}..{it.max()} QPs with a wrong mask {wrong.tolist()[:8]}")
    assert (st == OK).all(), (what, st)
    assert np.array_equal(mask, want), (what, wrong, [np.nonzero(mask[i])[0].tolist() for i in wrong[:4]])
    assert el.max() <= X_TOL, (what, el)
    rest = lam.copy()
    rest[k, h.row] = 0.0
    if meq:
        scale = 1.0 + np.abs(lam_eq).max(axis=1, keepdims=True)
        assert (np.abs(rest[:, :meq] - lam_eq) <= X_TOL * scale).all(), what
        rest[:, :meq] = 0.0
    assert (rest == 0.0).all(), (what, np.nonzero(rest))
    assert ex.max() <= X_TOL, (what, ex)
    assert it.min() == it.max(), (what, it)
    if iters is not None:
        assert it[0] == iters, (what, it[0], iters)


@pytest.mark.parametrize("route", P.ONE_HOT, ids=[r[0] for r in P.ONE_HOT])
def test_one_hot_rows(qpb, route):
    """m QPs in one launch, QP k with row k alone active: every dense route,
    (12, 65) (gi_gram with a third `active` word holding one row) and
    (128, 256) (its full tile set, eight words)."""
    name, n, m, _, flags = route
    h = P.one_hot_rows(n, m, P.seed_of(n, m))
    sol = _host(qpb.solve(*_dev(*h.tiled()), flags=flags))
    _check(qpb, h, sol, name, iters=None if flags & P.FLAG_MIXED else 2)


@pytest.mark.parametrize("n", P.ONE_HOT_BOX_N)
def test_one_hot_bounds(qpb, n):
    """qpb_solve_box, 2n QPs: QP j with upper bound j alone active, QP n + j
    with lower bound j.  The mask is the 2n x 2n identity in qpb.h's
    upper-then-lower order: every `active` word, up to eight at n = 128."""
    h, lb, ub = P.one_hot_bounds(n, P.seed_of(n, 2 * n))
    H, f, _, _ = h.tiled()
    sol = _host(qpb.solve_box(*_dev(H, f, lb, ub)))
    _check(qpb, h, sol, f"box n={n}", iters=2)


@pytest.mark.parametrize("n,m,meq,B", P.EQ)
def test_one_hot_eq(qpb, n, m, meq, B):
    """qpb_solve_eq with the one-hot row ranging over the inequality rows; the
    meq equalities are tight at the unconstrained minimiser, so they are taken
    with a zero step.  The closed form is the projection inside the
    equalities' null space (planted.one_hot_eq; its precondition holds at both
    shapes, tests/test_planted.py).  The equality bits are set, the inequality
    mask is one-hot, x and the multipliers meet the closed form; iters is the
    same for the whole launch: meq + 2 (each equality taken is one)."""
    h, lam_eq = P.one_hot_eq(n, m, meq, P.seed_of(n, m) + meq)
    sol = _host(qpb.solve_eq(*_dev(*h.tiled()), meq))
    _check(qpb, h, sol, f"eq ({n},{m},{meq})", iters=meq + 2, meq=meq, lam_eq=lam_eq)
