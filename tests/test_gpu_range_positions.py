"""Every row index as the one active row, on each side, on the two-sided routes.

`active` and `lower` are written in 32-bit words and the dense form keeps one
or two rows per lane; a `lower` bit or a lam written one slot off shows only
when that one row is the active one.  tests/planted.py's one_hot_range makes a
launch of 2 (m - meq) QPs sharing H, f and A: QP k violates the upper side of
row meq + k alone at the unconstrained minimiser, QP (m - meq) + k its lower
side alone, every other bound keeps a slack above 0.5 at the closed-form
solution, and the equalities are tight at the unconstrained minimiser:

  status OK
  active == the identity pattern plus the equality bits, bit for bit
  lower clear in the upper half of the launch, the identity pattern in the lower half
  lam on the one row within 1e-9 relative of the signed closed form
    +-1 / (ar Hr^{-1} ar), every other inequality lam == 0.0, the equalities'
    within 1e-9 of the multipliers stationarity gives
  x within 1e-9 relative of the closed form
  iters equal across each half of the launch (printed)

through qpb_solve_range on every RANGE route, through
qpb_solve_range_factored on the same launches (H and A are shared already),
and, with the last n rows the identity, through qpb_solve_range_box on every
RANGE_BOX route: every G row and every variable bound is in turn the one
active row on each side, and every output equals qpb_solve_range's on [G; I]
bit for bit.

Measured on the MI355X (measurements, not bars): over all routes and the three
entry points x err <= 2.1e-15 and lam err <= 5.8e-15, no wrong bit.  iters is
the same in both halves of every launch and the same factored and unfactored,
meq + 2 on every route (each equality taken is one trip, the one row another,
and one trip finds nothing; tests/test_gpu_positions.py's count).
"""
import numpy as np
import pytest

import planted as P
import range_oracle as RO

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

X_TOL = 1e-9
OK = 0
NAMES = ("x", "lam", "active", "lower", "status", "iters")


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    return q


def _dev(*arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
            for a in arrays]


def _host(sol):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in sol]


def _check(h, sol, what, meq):
    x, lam, act, low, st, it = sol
    Q, m = h.bl.shape
    K = Q // 2
    mask, lmask = RO.unpack_bits(act, m), RO.unpack_bits(low, m)
    want = h.mask()
    want_low = want & h.lower[:, None]
    want[:, :meq] = True
    k = np.arange(Q)
    ex = np.abs(x - h.x).max(axis=1) / np.maximum(1.0, np.abs(h.x).max(axis=1))
    el = np.abs(lam[k, h.row] - h.lam) / np.abs(h.lam)
    wrong = np.nonzero((mask != want).any(axis=1) | (lmask != want_low).any(axis=1))[0]
    print(f"{what}: {Q} QPs, status {np.bincount(st, minlength=5).tolist()} x err {ex.max():.2e} "
          f"lam err {el.max():.2e} iters upper half {it[:K].min()}..{it[:K].max()} lower half "
          f"{it[K:].min()}..{it[K:].max()} QPs with a wrong bit {wrong.tolist()[:8]}")
    assert (st == OK).all(), (what, st)
    assert np.array_equal(mask, want), (what, wrong, [np.nonzero(mask[i])[0].tolist() for i in wrong[:4]])
    assert not lmask[:K].any(), (what, np.nonzero(lmask[:K]))
    assert np.array_equal(lmask, want_low), (what, wrong, [np.nonzero(lmask[i])[0].tolist() for i in wrong[:4]])
    assert el.max() <= X_TOL, (what, el)
    assert np.array_equal(np.sign(lam[k, h.row]), np.where(h.lower, -1.0, 1.0)), what
    rest = lam.copy()
    rest[k, h.row] = 0.0
    if meq:
        scale = 1.0 + np.abs(h.lam_eq).max(axis=1, keepdims=True)
        assert (np.abs(rest[:, :meq] - h.lam_eq) <= X_TOL * scale).all(), what
        rest[:, :meq] = 0.0
    assert (rest == 0.0).all(), (what, np.nonzero(rest))
    assert ex.max() <= X_TOL, (what, ex)
    assert it[:K].min() == it[:K].max() and it[K:].min() == it[K:].max(), (what, it)


@pytest.mark.parametrize("n,m,meq,B", P.RANGE)
def test_one_hot_range(qpb, n, m, meq, B):
    """qpb_solve_range, and the same launch through qpb_solve_range_factored."""
    h = P.one_hot_range(n, m, meq, P.seed_of(n, m) + meq)
    H, f, A, bl, bu = h.tiled()
    _check(h, _host(qpb.solve_range(*_dev(H, f, A, bl, bu), meq)), f"range ({n},{m},{meq})", meq)
    F = qpb.factor_shared(*_dev(h.H, h.A))
    sol = _host(qpb.solve_range_factored(F, *_dev(f, bl, bu), meq))
    assert int(F.status.cpu().numpy()[0]) == OK
    _check(h, sol, f"range factored ({n},{m},{meq})", meq)


@pytest.mark.parametrize("n,mg,meq,B", P.RANGE_BOX)
def test_one_hot_range_box(qpb, n, mg, meq, B):
    """qpb_solve_range_box with every G row and every variable bound in turn
    the one active row on each side; bit for bit qpb_solve_range on [G; I]."""
    m = mg + n
    h = P.one_hot_range(n, m, meq, P.seed_of(n, m) + meq, box_rows=n)
    H, f, A, bl, bu = h.tiled()
    assert np.array_equal(A[:, mg:], np.broadcast_to(np.eye(n), (len(f), n, n)))
    G, gl, gu = (A[:, :mg], bl[:, :mg], bu[:, :mg]) if mg else (None, None, None)
    box = _host(qpb.solve_range_box(*_dev(H, f, G, gl, gu, bl[:, mg:], bu[:, mg:]), meq))
    _check(h, box, f"range_box ({n},{mg},{meq})", meq)
    mat = _host(qpb.solve_range(*_dev(H, f, A, bl, bu), meq))
    bad = [name for name, u, v in zip(NAMES, box, mat) if not np.array_equal(u.view(np.uint8), v.view(np.uint8))]
    assert not bad, bad
