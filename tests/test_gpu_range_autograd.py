"""qpb.diff.solve_range on the GPU: torch autograd through the range solve.

loss = (w . x).sum() through qpb.diff.solve_range; .backward() is compared
with the test's own central difference (eps = 1e-6) of qpb.solve_range along one
seeded direction that moves all of H (symmetrised), f, A, bl and bu at once.
The bar is 1e-4 relative, as in tests/test_gpu_autograd.py: on these shapes the
CPU oracle finds every active |lam| >= 13 and every inactive slack >= 0.023
(re-asserted below), which keeps `active` and `lower` fixed at +-eps; the
margin covers the noise of a finite difference of fp64 solves.
"""
import numpy as np
import pytest

import range_oracle as RO

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

EPS = 1e-6
SHAPES = [(5, 8, 0, 4), (20, 40, 2, 4)]  # n, m, meq, B


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    import qpb.diff  # noqa: F401
    return q


def _dev(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda().requires_grad_(grad)


def _margins(n, m, meq, Bq):
    """(smallest active |lam| over the rows >= meq, smallest inactive slack on
    either side) of the reference batch."""
    H, f, A, bl, bu, _, refs = RO.range_reference(Bq, n, m, meq)
    lam_min, slack_min = np.inf, np.inf
    for i, r in enumerate(refs):
        ax = A[i] @ r.x
        for j in range(meq, m):
            if r.active[j]:
                lam_min = min(lam_min, abs(r.lam[j]))
                slack_min = min(slack_min, (ax[j] - bl[i, j]) if not r.lower[j] else (bu[i, j] - ax[j]))
            else:
                slack_min = min(slack_min, bu[i, j] - ax[j], ax[j] - bl[i, j])
    return lam_min, slack_min


@pytest.mark.parametrize("n,m,meq,Bq", SHAPES)
def test_backward_matches_a_central_difference(qpb, n, m, meq, Bq):
    H, f, A, bl, bu, _, refs = RO.range_reference(Bq, n, m, meq)
    lam_min, slack_min = _margins(n, m, meq, Bq)
    print(f"({n},{m},{meq}) B={Bq}: smallest active |lam| {lam_min:.3g}, smallest inactive slack {slack_min:.3g}")
    # the two figures at the two digits they are stated with (12.96 and 0.02297 on the (20, 40, 2) shape)
    assert float(f"{lam_min:.2g}") >= 13.0 and float(f"{slack_min:.2g}") >= 0.023
    rng = np.random.default_rng([11, n, m])
    w = rng.standard_normal((Bq, n))
    dH = rng.standard_normal((Bq, n, n))
    dH = 0.5 * (dH + dH.transpose(0, 2, 1))
    df, dA = rng.standard_normal((Bq, n)), rng.standard_normal((Bq, m, n))
    dl, du = rng.standard_normal((Bq, m)), rng.standard_normal((Bq, m))
    Ht, ft, At, lt, ut = (_dev(v, True) for v in (H, f, A, bl, bu))
    x, status = qpb.diff.solve_range(Ht, ft, At, lt, ut, meq)
    assert not status.requires_grad and (status == qpb.OK).all()
    (_dev(w) * x).sum().backward()
    torch.cuda.synchronize()
    ana = sum(float((t.grad.cpu().numpy() * d).sum())
              for t, d in ((Ht, dH), (ft, df), (At, dA), (lt, dl), (ut, du)))

    def value(s):
        sol = qpb.solve_range(_dev(H + s * dH), _dev(f + s * df), _dev(A + s * dA), _dev(bl + s * dl),
                              _dev(bu + s * du), meq)
        torch.cuda.synchronize()
        assert (sol.status == qpb.OK).all()
        return float((w * sol.x.cpu().numpy()).sum()), sol.active.cpu().numpy(), sol.lower.cpu().numpy()

    (lp, ap, wp), (lm, am, wm) = value(EPS), value(-EPS)
    num = (lp - lm) / (2 * EPS)
    rel = abs(ana - num) / (1.0 + abs(num))
    print(f"({n},{m},{meq}) B={Bq}: autograd {ana:.9e} central difference {num:.9e} relative {rel:.2e}")
    assert np.array_equal(ap, am) and np.array_equal(wp, wm)  # the same sets on both sides
    assert rel <= 1e-4
    assert np.array_equal(Ht.grad.cpu().numpy(), Ht.grad.cpu().numpy().transpose(0, 2, 1))
    assert (lt.grad != 0).any() and (ut.grad != 0).any()


@pytest.mark.parametrize("n,m,meq,Bq", SHAPES)
def test_gb_is_routed_by_the_lower_bits(qpb, n, m, meq, Bq):
    H, f, A, bl, bu, _, _ = RO.range_reference(Bq, n, m, meq)
    Hd, fd, Ad = _dev(H), _dev(f), _dev(A)
    lt, ut = _dev(bl, True), _dev(bu, True)
    x, _ = qpb.diff.solve_range(Hd, fd, Ad, lt, ut, meq)
    w = _dev(np.random.default_rng([12, n, m]).standard_normal((Bq, n)))
    (w * x).sum().backward()
    sol = qpb.solve_range(Hd, fd, Ad, _dev(bl), _dev(bu), meq)
    _, _, _, gb = qpb.solve_backward(Hd, Ad, qpb.Solution(sol.x, sol.lam, sol.active, sol.status, None), w,
                                     need=("b",))
    torch.cuda.synchronize()
    low = RO.unpack_bits(sol.lower.cpu().numpy(), m)
    gl, gu, gb = lt.grad.cpu().numpy(), ut.grad.cpu().numpy(), gb.cpu().numpy()
    assert np.array_equal(gl + gu, gb)  # one of the two is an exact 0 everywhere
    assert np.array_equal(np.where(low, gb, 0.0), gl) and np.array_equal(np.where(low, 0.0, gb), gu)
    assert (gl[~low] == 0).all() and (gl[:, :meq] == 0).all() and (gu[low] == 0).all()
    assert low.any() and (gb != 0).any()


def test_a_shared_A_gets_the_summed_gradient(qpb):
    n, m, meq, Bq = 20, 40, 2, 4
    H, f, A, bl, bu, xc, _ = RO.range_reference(Bq, n, m, meq)
    A0 = A[0]
    ax = np.einsum("ij,bj->bi", A0, xc)
    rng = np.random.default_rng([13, n, m])
    buS = ax + rng.uniform(0.05, 1.0, size=ax.shape)
    blS = ax - rng.uniform(0.05, 1.0, size=ax.shape)
    blS[:, :meq] = buS[:, :meq] = ax[:, :meq]
    Hd, fd, At = _dev(H), _dev(f), _dev(A0, True)
    w = _dev(rng.standard_normal((Bq, n)))
    x, status = qpb.diff.solve_range(Hd, fd, At, _dev(blS), _dev(buS), meq)
    assert (status == qpb.OK).all()
    (w * x).sum().backward()
    sol = qpb.solve_range(Hd, fd, _dev(A0), _dev(blS), _dev(buS), meq)
    _, _, gA, _ = qpb.solve_shared_backward(Hd, _dev(A0), qpb.Solution(sol.x, sol.lam, sol.active, sol.status, None),
                                            w, need=("A",))
    torch.cuda.synchronize()
    assert tuple(At.grad.shape) == (m, n)
    assert torch.equal(At.grad, gA) and bool((gA != 0).any())


def test_a_bound_passed_as_none_gets_no_gradient(qpb):
    n, m, meq, Bq = 5, 8, 0, 4
    H, f, A, bl, bu, _, _ = RO.range_reference(Bq, n, m, meq)
    for which in ("bl", "bu"):
        ft, lt, ut = _dev(f, True), _dev(bl, True), _dev(bu, True)
        x, status = qpb.diff.solve_range(_dev(H), ft, _dev(A), None if which == "bl" else lt,
                                         None if which == "bu" else ut, meq)
        assert (status == qpb.OK).all()
        x.sum().backward()
        torch.cuda.synchronize()
        assert ft.grad is not None
        assert (lt.grad is None) == (which == "bl") and (ut.grad is None) == (which == "bu")
    # a bound that does not require grad gets none either
    lt, ut = _dev(bl), _dev(bu, True)
    x, _ = qpb.diff.solve_range(_dev(H), _dev(f), _dev(A), lt, ut, meq)
    x.sum().backward()
    assert lt.grad is None and ut.grad is not None


def test_forward_raises_above_the_limit(qpb):
    import eq_oracle as EO
    n, m, Bq = 40, 80, 2
    H, f, A, b, xc = EO.eq_family(11, Bq, n, m, 0)
    with pytest.raises(qpb.QPBError) as e:
        qpb.diff.solve_range(_dev(H), _dev(f, True), _dev(A), _dev(b - 1.0), _dev(b))
    assert e.value.code == qpb.ERR_UNSUPPORTED
