"""qpb.diff.solve(..., prefactor=True) on the GPU: the forward factors the one H
and A and solves with qpb.solve_factored, the backward is the unchanged
qpb.solve_shared_backward on that solution.  Everything is compared bit for bit
with the calls it is made of; the default, prefactor=False, stays today's call.
"""
import numpy as np
import pytest

import shared_cases as SC

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    import qpb.diff  # noqa: F401
    return q


def _dev(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda().requires_grad_(grad)


@pytest.mark.parametrize("n,m,meq", [(5, 9, 2), (16, 32, 4), (20, 40, 4)])
def test_prefactor_is_factor_solve_and_the_shared_backward(qpb, n, m, meq):
    B = 5
    H0, f, A0, b = SC.family(B, n, m, meq)
    w = np.random.default_rng([SC.SEED, n, m]).standard_normal((B, n))
    Ht, ft, At, bt = (_dev(v, True) for v in (H0, f, A0, b))
    x, status = qpb.diff.solve(Ht, ft, At, bt, meq, prefactor=True)
    assert not status.requires_grad and (status == qpb.OK).all()
    sol = qpb.solve_factored(qpb.factor_shared(_dev(H0), _dev(A0)), _dev(f), _dev(b), meq)
    torch.cuda.synchronize()
    assert np.array_equal(x.detach().cpu().numpy(), sol.x.cpu().numpy())
    assert np.array_equal(status.cpu().numpy(), sol.status.cpu().numpy())
    loss = (_dev(w) * x).sum()
    loss.backward()
    gH, gf, gA, gb = qpb.solve_shared_backward(_dev(H0), _dev(A0), sol, _dev(w))
    torch.cuda.synchronize()
    for t, g, shape in ((Ht, gH, (n, n)), (ft, gf, (B, n)), (At, gA, (m, n)), (bt, gb, (B, m))):
        assert tuple(t.grad.shape) == shape
        assert np.array_equal(t.grad.cpu().numpy(), g.cpu().numpy()), shape


def test_prefactor_without_rows(qpb):
    n, B = 3, 5
    H0, f, _, _ = SC.family(B, n, 0, 0)
    Ht, ft = _dev(H0, True), _dev(f, True)
    x, status = qpb.diff.solve(Ht, ft, prefactor=True)
    x.sum().backward()
    torch.cuda.synchronize()
    assert (status == qpb.OK).all()
    assert np.allclose(x.detach().cpu().numpy(), np.linalg.solve(H0, -f.T).T, rtol=1e-12, atol=1e-12)
    assert tuple(Ht.grad.shape) == (n, n) and tuple(ft.grad.shape) == (B, n)


def test_prefactor_needs_one_matrix_for_the_batch(qpb):
    n, m, meq, B = 16, 32, 4, 5
    H0, f, A0, b = SC.family(B, n, m, meq)
    with pytest.raises(ValueError):
        qpb.diff.solve(_dev(SC.expand(H0, B)), _dev(f), _dev(A0), _dev(b), meq, prefactor=True)
    with pytest.raises(ValueError):
        qpb.diff.solve(_dev(H0), _dev(f), _dev(SC.expand(A0, B)), _dev(b), meq, prefactor=True)


@pytest.mark.parametrize("shared_h,shared_a", [(True, True), (False, True), (False, False)])
def test_the_default_is_unchanged(qpb, shared_h, shared_a):
    """prefactor=False, and no prefactor at all: the outputs and gradients of
    qpb.solve_shared / qpb.solve_eq and their backward, bit for bit."""
    n, m, meq, B = 16, 32, 4, 5
    H0, f, A0, b = SC.family(B, n, m, meq)
    Hn, An = SC.operand(H0, B, shared_h), SC.operand(A0, B, shared_a)
    w = np.random.default_rng([SC.SEED, 1]).standard_normal((B, n))
    sol = qpb.solve_shared(_dev(Hn), _dev(f), _dev(An), _dev(b), meq)
    back = qpb.solve_shared_backward if (shared_h or shared_a) else qpb.solve_backward
    want = back(_dev(Hn), _dev(An), sol, _dev(w))
    torch.cuda.synchronize()
    for kw in ({}, {"prefactor": False}):
        ins = [_dev(v, True) for v in (Hn, f, An, b)]
        x, status = qpb.diff.solve(*ins, meq, **kw)
        (_dev(w) * x).sum().backward()
        torch.cuda.synchronize()
        assert np.array_equal(x.detach().cpu().numpy(), sol.x.cpu().numpy())
        assert np.array_equal(status.cpu().numpy(), sol.status.cpu().numpy())
        for t, g in zip(ins, want):
            assert np.array_equal(t.grad.cpu().numpy(), g.cpu().numpy())
