"""qpb.diff.solve with a 2-D H and A -- one matrix each for the whole batch, the
weights of a QP layer -- against the same call on ``.expand(B, ...)`` views:
x is bitwise equal, f.grad and b.grad are bitwise equal, H.grad (n, n) and
A.grad (m, n) agree with the expanded call's (autograd's sum of the per-QP
gradients) within the derived bound of tests/shared_cases.py on both sides.
And the point of the feature: at B = 16 384, n = 16, m = 32 the 2-D forward
and backward never allocate a (B, n, n) tensor -- torch's peak stays below
B n n 8 bytes = 33.5 MB (the outputs are about 13 MB by shape).
"""
import numpy as np
import pytest

import shared_cases as SC
from bwd_harness import dev as _dev

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    import qpb.diff  # noqa: F401
    return q


def _leaves(H0, f, A0, b):
    return [_dev(a).requires_grad_(True) for a in (H0, f, A0, b)]


@pytest.mark.parametrize("n,m,meq", [(5, 9, 2), (16, 32, 4), (20, 40, 4)])
def test_two_d_operands_against_expanded(qpb, n, m, meq):
    B = SC.batches(qpb)[-1]
    H0, f, A0, b = SC.family(B, n, m, meq)
    w = _dev(np.random.default_rng([SC.SEED, n, m]).standard_normal((B, n)))
    H2, f2, A2, b2 = _leaves(H0, f, A0, b)
    x2, st2 = qpb.diff.solve(H2, f2, A2, b2, meq)
    (w * x2).sum().backward()
    H3, f3, A3, b3 = _leaves(H0, f, A0, b)
    x3, st3 = qpb.diff.solve(H3.expand(B, n, n), f3, A3.expand(B, m, n), b3, meq)
    (w * x3).sum().backward()
    torch.cuda.synchronize()
    assert (st2.cpu().numpy() == 0).all()
    assert H2.grad.shape == (n, n) and A2.grad.shape == (m, n)
    eq = lambda a, c: np.array_equal(a.detach().cpu().numpy().view(np.uint8),  # noqa: E731
                                     c.detach().cpu().numpy().view(np.uint8))
    assert eq(x2, x3) and eq(st2, st3)
    assert eq(f2.grad, f3.grad) and eq(b2.grad, b3.grad)
    x, gf, gb = x2.detach().cpu().numpy(), f2.grad.cpu().numpy(), b2.grad.cpu().numpy()
    sol = qpb.solve_shared(_dev(H0), _dev(f), _dev(A0), _dev(b), meq)
    torch.cuda.synchronize()
    mask = qpb.active_mask_to_bool(sol.active.cpu().numpy(), m)
    bH, bA = SC.sum_bound(x, gf, gb, sol.lam.cpu().numpy(), mask, np.ones(B, bool))
    dH = np.abs(H2.grad.cpu().numpy() - H3.grad.cpu().numpy())
    dA = np.abs(A2.grad.cpu().numpy() - A3.grad.cpu().numpy())
    with np.errstate(invalid="ignore", divide="ignore"):
        print(f"n={n} m={m}: worst |delta| / bound: H {np.nanmax(np.where(bH > 0, dH / bH, 0)):.3g}, "
              f"A {np.nanmax(np.where(bA > 0, dA / bA, 0)):.3g}")
    assert (dH <= bH).all() and (dA <= bA).all()
    g = H2.grad.cpu().numpy()
    assert np.array_equal(g, g.T)


def test_no_per_qp_matrix_is_allocated(qpb):
    B, n, m, meq = 16384, 16, 32, 0
    H0, _, A0, _ = SC.family(67, n, m, meq)
    rs = np.random.default_rng(SC.SEED)
    torch.cuda.synchronize()
    foreign = torch.cuda.memory_allocated()  # what other tests of the session still hold: not this call's
    xc = rs.uniform(-20.0, 20.0, size=(B, n))
    f = _dev(rs.uniform(-1e3, 1e3, size=(B, n))).requires_grad_(True)
    b = _dev(xc @ A0.T + rs.uniform(1.0, 10.0, size=(B, m))).requires_grad_(True)
    H, A = _dev(H0).requires_grad_(True), _dev(A0).requires_grad_(True)
    w = torch.ones((B, n), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    x, st = qpb.diff.solve(H, f, A, b, meq)
    (w * x).sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - foreign  # this test's inputs included
    print(f"peak over the 2-D forward and backward: {peak / 1e6:.1f} MB, "
          f"{(torch.cuda.max_memory_allocated() - base) / 1e6:.1f} MB of it new "
          f"(a (B, n, n) tensor: {B * n * n * 8 / 1e6:.1f} MB)")
    assert peak < B * n * n * 8
    assert H.grad.shape == (n, n) and A.grad.shape == (m, n) and f.grad.shape == (B, n)
    assert (st == 0).all() and torch.isfinite(H.grad).all() and torch.isfinite(A.grad).all()
