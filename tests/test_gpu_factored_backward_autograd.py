"""qpb.diff.solve and qpb.diff.solve_range with prefactor=True on the GPU: the
backward factors the saved H and A once (qpb.factor_shared_backward) and runs
qpb.solve_factored_backward.  With qpb.solve_shared_backward patched to raise,
the gradients still come, and they equal the unpatched call's bit for bit; with
prefactor=False the patched function is the one that is called.
"""
import numpy as np
import pytest

import shared_cases as SC

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SHAPES = [(5, 9, 2), (16, 32, 4), (20, 40, 4)]
B = 5


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    import qpb.diff  # noqa: F401
    return q


def _dev(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda().requires_grad_(grad)


class Called(Exception):
    pass


def _raise(*a, **kw):
    raise Called("qpb.solve_shared_backward")


def _same(t, g, shape):
    assert tuple(t.grad.shape) == shape
    assert np.array_equal(t.grad.cpu().numpy().view(np.uint8), g.cpu().numpy().view(np.uint8)), shape


@pytest.mark.parametrize("n,m,meq", SHAPES)
def test_solve_prefactor_runs_the_factored_backward(qpb, monkeypatch, n, m, meq):
    H0, f, A0, b = SC.family(B, n, m, meq)
    w = np.random.default_rng([SC.SEED, n, m, 17]).standard_normal((B, n))
    sol = qpb.solve_factored(qpb.factor_shared(_dev(H0), _dev(A0)), _dev(f), _dev(b), meq)
    want = qpb.solve_shared_backward(_dev(H0), _dev(A0), sol, _dev(w))
    torch.cuda.synchronize()
    monkeypatch.setattr(qpb, "solve_shared_backward", _raise)
    Ht, ft, At, bt = (_dev(v, True) for v in (H0, f, A0, b))
    x, status = qpb.diff.solve(Ht, ft, At, bt, meq, prefactor=True)
    assert (status == qpb.OK).all()
    (_dev(w) * x).sum().backward()
    torch.cuda.synchronize()
    for t, g, shape in zip((Ht, ft, At, bt), want, ((n, n), (B, n), (m, n), (B, m))):
        _same(t, g, shape)
    # a subset of the inputs: only f and b want gradients
    ft2, bt2 = _dev(f, True), _dev(b, True)
    x, _ = qpb.diff.solve(_dev(H0), ft2, _dev(A0), bt2, meq, prefactor=True)
    (_dev(w) * x).sum().backward()
    torch.cuda.synchronize()
    _same(ft2, want[1], (B, n))
    _same(bt2, want[3], (B, m))
    # the default is the patched call
    ins = [_dev(v, True) for v in (H0, f, A0, b)]
    x, _ = qpb.diff.solve(*ins, meq, prefactor=False)
    with pytest.raises(Called):
        (_dev(w) * x).sum().backward()


@pytest.mark.parametrize("n,m,meq", SHAPES)
def test_solve_range_prefactor_runs_the_factored_backward(qpb, monkeypatch, n, m, meq):
    H0, f, A0, b = SC.family(B, n, m, meq)
    bl = b - np.random.default_rng([SC.SEED, n, m, 18]).uniform(10.0, 50.0, size=b.shape)  # at least the family's slack
    w = np.random.default_rng([SC.SEED, n, m, 19]).standard_normal((B, n))
    sol = qpb.solve_range_factored(qpb.factor_shared(_dev(H0), _dev(A0)), _dev(f), _dev(bl), _dev(b), meq)
    bsol = qpb.Solution(sol.x, sol.lam, sol.active, sol.status, None)
    gH, gf, gA, gb = qpb.solve_shared_backward(_dev(H0), _dev(A0), bsol, _dev(w))
    torch.cuda.synchronize()
    monkeypatch.setattr(qpb, "solve_shared_backward", _raise)
    Ht, ft, At, blt, but = (_dev(v, True) for v in (H0, f, A0, bl, b))
    x, status = qpb.diff.solve_range(Ht, ft, At, blt, but, meq, prefactor=True)
    assert (status == qpb.OK).all()
    (_dev(w) * x).sum().backward()
    torch.cuda.synchronize()
    _same(Ht, gH, (n, n))
    _same(ft, gf, (B, n))
    _same(At, gA, (m, n))
    # gb goes to bl where the row's `lower` bit is set, to bu elsewhere: the two add up to it, element by element
    low = qpb.active_mask_to_bool(sol.lower.cpu().numpy(), m)
    gbn = gb.cpu().numpy()
    assert np.array_equal(blt.grad.cpu().numpy().view(np.uint8), np.where(low, gbn, 0.0).view(np.uint8))
    assert np.array_equal(but.grad.cpu().numpy().view(np.uint8), np.where(low, 0.0, gbn).view(np.uint8))
    ins = [_dev(v, True) for v in (H0, f, A0, bl, b)]
    x, _ = qpb.diff.solve_range(*ins, meq, prefactor=False)
    with pytest.raises(Called):
        (_dev(w) * x).sum().backward()


def test_a_forward_without_gradients_factors_nothing_for_the_backward(qpb, monkeypatch):
    n, m, meq = 16, 32, 4
    H0, f, A0, b = SC.family(B, n, m, meq)

    def never(*a, **kw):
        raise AssertionError("qpb.factor_shared_backward called in a forward")

    monkeypatch.setattr(qpb, "factor_shared_backward", never)
    x, status = qpb.diff.solve(_dev(H0, True), _dev(f, True), _dev(A0), _dev(b), meq, prefactor=True)
    with torch.no_grad():
        x2, _ = qpb.diff.solve(_dev(H0), _dev(f), _dev(A0), _dev(b), meq, prefactor=True)
    torch.cuda.synchronize()
    assert (status == qpb.OK).all() and np.array_equal(x.detach().cpu().numpy(), x2.cpu().numpy())
