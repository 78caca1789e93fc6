"""qpb.diff.solve_box on the GPU: torch autograd through the box solver.

loss = (w . x).sum() through qpb.diff.solve_box; .backward() is compared with
the test's own central difference (eps = 1e-6) of qpb.solve_box along one
seeded direction that moves all of H (symmetrised), f, lb and ub at once.  The
bar is 1e-4 relative, as in tests/test_gpu_autograd.py: at width 10 every
active multiplier is >= 0.19 and every inactive slack >= 1e-2
(tests/test_box_bwd_oracle.py), which keeps the active set fixed at +-eps; the
margin covers the noise of a finite difference of fp64 solves.
"""
import numpy as np
import pytest

import box_bwd_oracle as BO

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

EPS = 1e-6
SEED = 11
WIDTH = 10.0


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    import qpb.diff  # noqa: F401
    return q


def _dev(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda().requires_grad_(grad)


@pytest.mark.parametrize("n,Bq", [(5, 4), (20, 3)])
def test_backward_matches_a_central_difference(qpb, n, Bq):
    H, f, lb, ub = BO.family(SEED, Bq, n, WIDTH)
    rng = np.random.default_rng([SEED, n])
    w = rng.standard_normal((Bq, n))
    dH = rng.standard_normal((Bq, n, n))
    dH = 0.5 * (dH + dH.transpose(0, 2, 1))
    df, dl, du = rng.standard_normal((Bq, n)), rng.standard_normal((Bq, n)), rng.standard_normal((Bq, n))
    Ht, ft, lt, ut = (_dev(v, True) for v in (H, f, lb, ub))
    x, status = qpb.diff.solve_box(Ht, ft, lt, ut)
    assert not status.requires_grad and (status == qpb.OK).all()
    loss = (_dev(w) * x).sum()
    loss.backward()
    torch.cuda.synchronize()
    ana = sum(float((t.grad.cpu().numpy() * d).sum()) for t, d in ((Ht, dH), (ft, df), (lt, dl), (ut, du)))

    def value(s):
        sol = qpb.solve_box(_dev(H + s * dH), _dev(f + s * df), _dev(lb + s * dl), _dev(ub + s * du))
        torch.cuda.synchronize()
        assert (sol.status == qpb.OK).all()
        return float((w * sol.x.cpu().numpy()).sum()), sol.active.cpu().numpy()

    (lp, ap), (lm, am) = value(EPS), value(-EPS)
    num = (lp - lm) / (2 * EPS)
    rel = abs(ana - num) / (1.0 + abs(num))
    mask = qpb.active_mask_to_bool(ap, 2 * n)
    print(f"n={n} B={Bq}: autograd {ana:.9e} central difference {num:.9e} relative {rel:.2e} "
          f"active upper {mask[:, :n].sum()} lower {mask[:, n:].sum()}")
    assert np.array_equal(ap, am)  # the same active set on both sides
    assert mask[:, :n].any() and mask[:, n:].any()  # both bounds' gradients take part
    assert rel <= 1e-4
    assert np.array_equal(Ht.grad.cpu().numpy(), Ht.grad.cpu().numpy().transpose(0, 2, 1))


def test_only_the_wanted_gradients_are_computed(qpb):
    n, Bq = 5, 4
    H, f, lb, ub = BO.family(SEED, Bq, n, WIDTH)
    Ht, lt, ut = _dev(H), _dev(lb), _dev(ub)
    ft = _dev(f, True)
    x, status = qpb.diff.solve_box(Ht, ft, lt, ut)
    x.sum().backward()
    torch.cuda.synchronize()
    assert Ht.grad is None and lt.grad is None and ut.grad is None
    H2, f2, l2, u2 = (_dev(v, True) for v in (H, f, lb, ub))
    x2, _ = qpb.diff.solve_box(H2, f2, l2, u2)
    x2.sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(ft.grad, f2.grad) and H2.grad is not None and l2.grad is not None and u2.grad is not None
    # the binding itself: only what `need` names is allocated and returned
    sol = qpb.solve_box(Ht, _dev(f), lt, ut)
    got = qpb.solve_box_backward(Ht, sol, torch.ones_like(sol.x), need=("lb",))
    torch.cuda.synchronize()
    assert [t is None for t in got] == [True, True, False, True] and torch.equal(got[2], l2.grad)


@pytest.mark.parametrize("absent", ["lb", "ub"])
def test_one_sided_boxes(qpb, absent):
    """A bound passed as None gets no gradient, and the other bound's gradient
    is that of the two-sided call whose bounds on that side are absent (+-inf)."""
    n, Bq = 5, 4
    H, f, lb, ub = BO.family(SEED, Bq, n, WIDTH)
    inf = np.full((Bq, n), -np.inf if absent == "lb" else np.inf)
    Ht, ft = _dev(H, True), _dev(f, True)
    kept = _dev(ub if absent == "lb" else lb, True)
    args = (None, kept) if absent == "lb" else (kept, None)
    x, status = qpb.diff.solve_box(Ht, ft, *args)
    assert (status == qpb.OK).all()
    x.sum().backward()
    H2, f2, kept2, inf2 = _dev(H, True), _dev(f, True), _dev(ub if absent == "lb" else lb, True), _dev(inf, True)
    args2 = (inf2, kept2) if absent == "lb" else (kept2, inf2)
    x2, status2 = qpb.diff.solve_box(H2, f2, *args2)
    assert (status2 == qpb.OK).all()
    x2.sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(x, x2)
    assert kept.grad is not None and bool((kept.grad != 0).any())
    assert torch.equal(kept.grad, kept2.grad) and torch.equal(Ht.grad, H2.grad) and torch.equal(ft.grad, f2.grad)
    assert bool((inf2.grad == 0).all())


def test_forward_runs_above_the_backward_limit(qpb):
    n, Bq = 40, 2
    H, f, lb, ub = BO.family(SEED, Bq, n, WIDTH)
    ft = _dev(f, True)
    x, status = qpb.diff.solve_box(_dev(H), ft, _dev(lb), _dev(ub))
    torch.cuda.synchronize()
    assert (status == qpb.OK).all() and x.requires_grad
    with pytest.raises(qpb.QPBError) as e:
        x.sum().backward()
    assert e.value.code == qpb.ERR_UNSUPPORTED
