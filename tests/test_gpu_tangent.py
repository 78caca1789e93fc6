"""qpb.solve_tangent on the GPU: the forward sensitivity (dx, dlam) of a solve
along a change (df, db) of f and b, one call of qpb_solve_backward_dual.

Compared with the test's own central difference (eps = 1e-6) of the GPU forward
qpb.solve_eq in (f, b), for x and for lam.  The bar is 1e-4 relative, the
constants of tests/test_gpu_autograd.py: strict complementarity keeps the
active set fixed at +-eps, the margin covers the noise of a finite difference
of fp64 solves.  db = None takes the existing kernels.
"""
import numpy as np
import pytest

import eq_oracle as EO

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

EPS = 1e-6
SEED = 11
B = 8


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    return q


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


@pytest.mark.parametrize("n,m,meq", [(5, 9, 2), (16, 32, 4), (20, 40, 4)])
def test_tangent_matches_a_central_difference(qpb, n, m, meq):
    H, f, A, b, xc = EO.eq_family(SEED, B, n, m, meq)
    rng = np.random.default_rng([SEED, n, m, 3])
    df, db = rng.standard_normal((B, n)), rng.standard_normal((B, m))
    Hd, Ad = _dev(H), _dev(A)
    sol = qpb.solve_eq(Hd, _dev(f), Ad, _dev(b), meq)
    dx, dlam = qpb.solve_tangent(Hd, Ad, sol, _dev(df), _dev(db))
    torch.cuda.synchronize()
    assert (sol.status == qpb.OK).all()
    mask = qpb.active_mask_to_bool(sol.active.cpu().numpy(), m)
    dx, dlam = dx.cpu().numpy(), dlam.cpu().numpy()
    assert (dlam[~mask] == 0.0).all()

    def side(s):
        p = qpb.solve_eq(Hd, _dev(f + s * df), Ad, _dev(b + s * db), meq)
        torch.cuda.synchronize()
        assert (p.status == qpb.OK).all() and torch.equal(p.active, sol.active)  # the same active set
        return p.x.cpu().numpy(), p.lam.cpu().numpy()

    (xp, lp), (xm, lm) = side(EPS), side(-EPS)
    nx, nl = (xp - xm) / (2 * EPS), (lp - lm) / (2 * EPS)
    ex = np.abs(dx - nx).max() / (1.0 + np.abs(nx).max())
    el = np.abs(dlam - nl).max() / (1.0 + np.abs(nl).max())
    print(f"({n},{m},{meq}): |tangent - central difference| / (1 + |cd|): x {ex:.2e} lam {el:.2e}")
    assert ex <= 1e-4 and el <= 1e-4


@pytest.mark.parametrize("n,m,meq", [(5, 9, 2), (16, 32, 4), (20, 40, 4)])
def test_no_db_is_the_existing_backward_bit_for_bit(qpb, n, m, meq):
    H, f, A, b, xc = EO.eq_family(SEED, B, n, m, meq)
    df = np.random.default_rng([SEED, n, m, 4]).standard_normal((B, n))
    Hd, Ad, dfd = _dev(H), _dev(A), _dev(df)
    sol = qpb.solve_eq(Hd, _dev(f), Ad, _dev(b), meq)
    dx, dlam = qpb.solve_tangent(Hd, Ad, sol, dfd)
    _, gf, _, gb = qpb.solve_backward(Hd, Ad, sol, dfd, need=("f", "b"))
    torch.cuda.synchronize()
    assert torch.equal(dx, gf) and torch.equal(dlam, -gb)
    assert np.array_equal(dx.cpu().numpy().view(np.uint8), gf.cpu().numpy().view(np.uint8))
    # a zero db through the DU form, on a side stream: every term the form adds is an exact zero
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    dx2, dlam2 = qpb.solve_tangent(Hd, Ad, sol, dfd, _dev(np.zeros((B, m))), stream=s)
    s.synchronize()
    assert torch.equal(dx2, dx) and torch.equal(dlam2, dlam)


def test_no_rows(qpb):
    """m = 0: dx = -H^{-1} df and there is no dlam."""
    n = 5
    H, f, *_ = EO.eq_family(SEED, B, n, 1, 0)
    df = np.random.default_rng(5).standard_normal((B, n))
    sol = qpb.solve(_dev(H), _dev(f))
    dx, dlam = qpb.solve_tangent(_dev(H), None, sol, _dev(df))
    torch.cuda.synchronize()
    ref = -np.linalg.solve(H, df[:, :, None])[:, :, 0]
    assert dlam is None
    assert np.abs(dx.cpu().numpy() - ref).max() <= 1e-6 * (1.0 + np.abs(ref).max())
