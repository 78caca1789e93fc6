"""qpb.diff.solve_dual and qpb.diff.solve_range_dual on the GPU: torch autograd
through a solve whose multipliers enter the loss.

loss = (w . x).sum() + (v . lam).sum(); .backward() is compared with the test's
own central difference (eps = 1e-6) of the forward along one seeded direction
that moves all of H (symmetrised), f, A and b (bl and bu) at once.  The bar is
1e-4 relative, the constants of tests/test_gpu_autograd.py and
tests/test_gpu_range_autograd.py, on their shapes and families: strict
complementarity keeps the active set (and `lower`) fixed at +-eps, the margin
covers the noise of a finite difference of fp64 solves.
"""
import numpy as np
import pytest

import eq_oracle as EO
import range_oracle as RO

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


def _direction(rng, Bq, n, m):
    dH = rng.standard_normal((Bq, n, n))
    return (0.5 * (dH + dH.transpose(0, 2, 1)), rng.standard_normal((Bq, n)), rng.standard_normal((Bq, m, n)),
            rng.standard_normal((Bq, m)))


@pytest.mark.parametrize("n,m,meq,Bq", [(3, 5, 1, 4), (16, 32, 4, 3), (20, 40, 4, 3)])
@pytest.mark.parametrize("reads", ["x and lam", "lam alone"])
def test_backward_matches_a_central_difference(qpb, n, m, meq, Bq, reads):
    H, f, A, b, xc = EO.eq_family(SEED, Bq, n, m, meq)
    rng = np.random.default_rng([SEED, n, m, 6])
    w, v = rng.standard_normal((Bq, n)), rng.standard_normal((Bq, m))
    if reads == "lam alone":
        w[:] = 0.0
    dH, df, dA, db = _direction(rng, Bq, n, m)
    Ht, ft, At, bt = (_dev(t, True) for t in (H, f, A, b))
    x, lam, status = qpb.diff.solve_dual(Ht, ft, At, bt, meq)
    assert not status.requires_grad and (status == qpb.OK).all() and lam.requires_grad
    loss = (_dev(v) * lam).sum() if reads == "lam alone" else (_dev(w) * x).sum() + (_dev(v) * lam).sum()
    loss.backward()
    torch.cuda.synchronize()
    ana = sum(float((t.grad.cpu().numpy() * d).sum()) for t, d in ((Ht, dH), (ft, df), (At, dA), (bt, db)))

    def value(s):
        sol = qpb.solve_eq(_dev(H + s * dH), _dev(f + s * df), _dev(A + s * dA), _dev(b + s * db), meq)
        torch.cuda.synchronize()
        assert (sol.status == qpb.OK).all()
        return float((w * sol.x.cpu().numpy()).sum() + (v * sol.lam.cpu().numpy()).sum()), sol.active.cpu().numpy()

    (lp, ap), (lm, am) = value(EPS), value(-EPS)
    num = (lp - lm) / (2 * EPS)
    rel = abs(ana - num) / (1.0 + abs(num))
    print(f"({n},{m},{meq}) B={Bq} {reads}: autograd {ana:.9e} central difference {num:.9e} relative {rel:.2e}")
    assert np.array_equal(ap, am)  # the same active set on both sides
    assert rel <= 1e-4
    assert np.array_equal(Ht.grad.cpu().numpy(), Ht.grad.cpu().numpy().transpose(0, 2, 1))


@pytest.mark.parametrize("n,m,meq,Bq", [(3, 5, 1, 4), (20, 40, 4, 3)])
def test_a_loss_in_x_alone_gives_solves_gradients_bit_for_bit(qpb, n, m, meq, Bq):
    H, f, A, b, xc = EO.eq_family(SEED, Bq, n, m, meq)
    w = _dev(np.random.default_rng([SEED, n, m, 7]).standard_normal((Bq, n)))
    one = [_dev(t, True) for t in (H, f, A, b)]
    x, status = qpb.diff.solve(*one, meq)
    (w * x).sum().backward()
    two = [_dev(t, True) for t in (H, f, A, b)]
    x2, lam2, _ = qpb.diff.solve_dual(*two, meq)
    (w * x2).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(x, x2)
    for a, c in zip(one, two):
        assert np.array_equal(a.grad.cpu().numpy().view(np.uint8), c.grad.cpu().numpy().view(np.uint8))


def test_shared_operands_get_summed_gradients(qpb):
    n, m, meq, Bq = 16, 32, 4, 5
    H, f, A, b, xc = EO.eq_family(SEED, Bq, n, m, meq)
    H0, A0 = H[0], A[0]
    slack = np.random.default_rng([SEED, 8]).uniform(1.0, 10.0, size=(Bq, m))
    slack[:, :meq] = 0.0
    bS = xc @ A0.T + slack
    rng = np.random.default_rng([SEED, 9])
    w, v = _dev(rng.standard_normal((Bq, n))), _dev(rng.standard_normal((Bq, m)))
    Ht, ft, At, bt = (_dev(t, True) for t in (H0, f, A0, bS))
    x, lam, status = qpb.diff.solve_dual(Ht, ft, At, bt, meq)
    assert (status == qpb.OK).all()
    ((w * x).sum() + (v * lam).sum()).backward()
    sol = qpb.solve_shared(_dev(H0), _dev(f), _dev(A0), _dev(bS), meq)
    gH, gf, gA, gb = qpb.solve_backward_dual(_dev(H0), _dev(A0), sol, w, v)
    torch.cuda.synchronize()
    assert tuple(Ht.grad.shape) == (n, n) and tuple(At.grad.shape) == (m, n)
    assert torch.equal(Ht.grad, gH) and torch.equal(At.grad, gA) and torch.equal(ft.grad, gf)
    assert torch.equal(bt.grad, gb) and bool((gA != 0).any())


@pytest.mark.parametrize("n,m,meq,Bq", [(5, 8, 0, 4), (20, 40, 2, 4)])
def test_range_backward_matches_a_central_difference(qpb, n, m, meq, Bq):
    H, f, A, bl, bu, _, refs = RO.range_reference(Bq, n, m, meq)
    rng = np.random.default_rng([SEED, n, m, 10])
    w, v = rng.standard_normal((Bq, n)), rng.standard_normal((Bq, m))
    dH, df, dA, dl = _direction(rng, Bq, n, m)
    du = rng.standard_normal((Bq, m))
    Ht, ft, At, lt, ut = (_dev(t, True) for t in (H, f, A, bl, bu))
    x, lam, status = qpb.diff.solve_range_dual(Ht, ft, At, lt, ut, meq)
    assert not status.requires_grad and (status == qpb.OK).all()
    ((_dev(w) * x).sum() + (_dev(v) * lam).sum()).backward()
    torch.cuda.synchronize()
    ana = sum(float((t.grad.cpu().numpy() * d).sum())
              for t, d in ((Ht, dH), (ft, df), (At, dA), (lt, dl), (ut, du)))

    def value(s):
        sol = qpb.solve_range(_dev(H + s * dH), _dev(f + s * df), _dev(A + s * dA), _dev(bl + s * dl),
                              _dev(bu + s * du), meq)
        torch.cuda.synchronize()
        assert (sol.status == qpb.OK).all()
        return (float((w * sol.x.cpu().numpy()).sum() + (v * sol.lam.cpu().numpy()).sum()),
                sol.active.cpu().numpy(), sol.lower.cpu().numpy())

    (lp, ap, wp), (lm, am, wm) = value(EPS), value(-EPS)
    num = (lp - lm) / (2 * EPS)
    rel = abs(ana - num) / (1.0 + abs(num))
    print(f"range ({n},{m},{meq}) B={Bq}: autograd {ana:.9e} central difference {num:.9e} relative {rel:.2e}")
    assert np.array_equal(ap, am) and np.array_equal(wp, wm)  # the same sets on both sides
    assert rel <= 1e-4
    # gbl / gbu land on the sides named by `lower`
    sol = qpb.solve_range(_dev(H), _dev(f), _dev(A), _dev(bl), _dev(bu), meq)
    _, _, _, gb = qpb.solve_backward_dual(_dev(H), _dev(A), qpb.Solution(sol.x, sol.lam, sol.active, sol.status, None),
                                          _dev(w), _dev(v), need=("b",))
    torch.cuda.synchronize()
    low = RO.unpack_bits(sol.lower.cpu().numpy(), m)
    gl, gu, gb = lt.grad.cpu().numpy(), ut.grad.cpu().numpy(), gb.cpu().numpy()
    assert np.array_equal(np.where(low, gb, 0.0), gl) and np.array_equal(np.where(low, 0.0, gb), gu)
    assert (gl[:, :meq] == 0).all() and low.any() and (gl != 0).any() and (gu != 0).any()


def test_range_loss_in_x_alone_is_solve_ranges_backward(qpb):
    n, m, meq, Bq = 5, 8, 0, 4
    H, f, A, bl, bu, _, _ = RO.range_reference(Bq, n, m, meq)
    w = _dev(np.random.default_rng([SEED, 11]).standard_normal((Bq, n)))
    one = [_dev(t, True) for t in (H, f, A, bl, bu)]
    x, _ = qpb.diff.solve_range(*one, meq)
    (w * x).sum().backward()
    two = [_dev(t, True) for t in (H, f, A, bl, bu)]
    x2, lam2, _ = qpb.diff.solve_range_dual(*two, meq)
    (w * x2).sum().backward()
    torch.cuda.synchronize()
    for a, c in zip(one, two):
        assert torch.equal(a.grad, c.grad)
    # a bound passed as None gets no gradient
    ft, ut = _dev(f, True), _dev(bu, True)
    x3, lam3, _ = qpb.diff.solve_range_dual(_dev(H), ft, _dev(A), None, ut, meq)
    (x3.sum() + lam3.sum()).backward()
    assert ft.grad is not None and ut.grad is not None
