"""qpb.diff on the GPU: torch autograd through the solver.

loss = (w . x).sum() through qpb.diff.solve; .backward() is compared with the
test's own central difference (eps = 1e-6) of qpb.solve_eq along one seeded
direction that moves all of H (symmetrised), f, A and b at once.  The bar is
1e-4 relative, as in tests/test_kkt_oracle.py: strict complementarity (>= 6e-3)
keeps the active set fixed at +-eps, the margin covers the noise of a finite
difference of fp64 solves.
"""
import numpy as np
import pytest

import eq_oracle as EO

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

EPS = 1e-6
SEED = 11


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    import qpb.diff  # noqa: F401
    return q


def _dev(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda().requires_grad_(grad)


@pytest.mark.parametrize("n,m,meq,Bq", [(3, 5, 1, 4), (20, 40, 4, 3)])
def test_backward_matches_a_central_difference(qpb, n, m, meq, Bq):
    H, f, A, b, xc = EO.eq_family(SEED, Bq, n, m, meq)
    rng = np.random.default_rng([SEED, n, m])
    w = rng.standard_normal((Bq, n))
    dH = rng.standard_normal((Bq, n, n))
    dH = 0.5 * (dH + dH.transpose(0, 2, 1))
    df, dA, db = rng.standard_normal((Bq, n)), rng.standard_normal((Bq, m, n)), rng.standard_normal((Bq, m))
    Ht, ft, At, bt = (_dev(v, True) for v in (H, f, A, b))
    x, status = qpb.diff.solve(Ht, ft, At, bt, meq)
    assert not status.requires_grad and (status == qpb.OK).all()
    loss = (_dev(w) * x).sum()
    loss.backward()
    torch.cuda.synchronize()
    ana = sum(float((t.grad.cpu().numpy() * d).sum()) for t, d in ((Ht, dH), (ft, df), (At, dA), (bt, db)))

    def value(s):
        sol = qpb.solve_eq(_dev(H + s * dH), _dev(f + s * df), _dev(A + s * dA), _dev(b + s * db), meq)
        torch.cuda.synchronize()
        assert (sol.status == qpb.OK).all()
        return float((w * sol.x.cpu().numpy()).sum()), sol.active.cpu().numpy()

    (lp, ap), (lm, am) = value(EPS), value(-EPS)
    num = (lp - lm) / (2 * EPS)
    rel = abs(ana - num) / (1.0 + abs(num))
    print(f"({n},{m},{meq}) B={Bq}: autograd {ana:.9e} central difference {num:.9e} relative {rel:.2e}")
    assert np.array_equal(ap, am)  # the same active set on both sides
    assert rel <= 1e-4
    assert np.array_equal(Ht.grad.cpu().numpy(), Ht.grad.cpu().numpy().transpose(0, 2, 1))


def test_only_the_wanted_gradients_are_computed(qpb):
    n, m, meq, Bq = 3, 5, 1, 4
    H, f, A, b, xc = EO.eq_family(SEED, Bq, n, m, meq)
    Ht, At, bt = _dev(H), _dev(A), _dev(b)
    ft = _dev(f, True)
    x, status = qpb.diff.solve(Ht, ft, At, bt, meq)
    x.sum().backward()
    torch.cuda.synchronize()
    assert Ht.grad is None and At.grad is None and bt.grad is None
    # dl/df = dx = -(K^{-1})_xx g with g = 1: compare with every gradient asked for
    H2, f2, A2, b2 = (_dev(v, True) for v in (H, f, A, b))
    x2, _ = qpb.diff.solve(H2, f2, A2, b2, meq)
    x2.sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(ft.grad, f2.grad) and H2.grad is not None and A2.grad is not None and b2.grad is not None


def test_no_rows(qpb):
    """m = 0: x = -H^{-1} f, so dl/df = -H^{-1} g."""
    n, Bq = 3, 4
    H, f, *_ = EO.eq_family(SEED, Bq, n, 1, 0)
    Ht, ft = _dev(H, True), _dev(f, True)
    x, status = qpb.diff.solve(Ht, ft)
    x.sum().backward()
    torch.cuda.synchronize()
    ref = -np.linalg.solve(H, np.ones((Bq, n, 1)))[:, :, 0]
    assert np.abs(ft.grad.cpu().numpy() - ref).max() <= 1e-6 * (1.0 + np.abs(ref).max())


def test_forward_runs_above_the_backward_limit(qpb):
    n, m, Bq = 40, 80, 2
    H, f, A, b, xc = EO.eq_family(SEED, Bq, n, m, 0)
    ft = _dev(f, True)
    x, status = qpb.diff.solve(_dev(H), ft, _dev(A), _dev(b))
    torch.cuda.synchronize()
    assert (status == qpb.OK).all() and x.requires_grad
    with pytest.raises(qpb.QPBError) as e:
        x.sum().backward()
    assert e.value.code == qpb.ERR_UNSUPPORTED
