"""qpb.diff.solve_range(..., prefactor=True) on the GPU: the forward factors the
one H and A and solves with qpb.solve_range_factored, the backward is the
unchanged qpb.solve_shared_backward on that solution with its gb routed to bl or
bu by the `lower` bits.

Three comparisons.  With the calls it is made of: bit for bit, as
tests/test_gpu_factored_autograd.py compares its pair of paths.  With
prefactor=False on the same 2-D H and A: x within the parity bar (1e-6), the same
`active` and `lower` (every QP of these batches is strictly complementary), and
the gradients within 1e-6 of their largest entry -- at a fixed active set dx and
dlam depend on H, A and the set alone, and the gradients are products of them
with x and lam (gH from dx x^T, gA from dlam x^T and lam dx^T, gf and gb dx and
dlam themselves), so the two paths' gradients differ by no more than their x and
lam do, relatively, which the parity bar holds to 1e-6.  With the test's own central
difference (eps = 1e-6) of qpb.solve_range_factored along one seeded direction
that moves H (symmetrised), f, A, bl and bu at once, at one shape of each kernel
class, as tests/test_gpu_range_autograd.py does: the bar is its 1e-4 relative.
On these shapes the CPU oracle finds every active |lam| >= 160 and every
inactive slack >= 0.03 (re-asserted below), which keeps `active` and `lower`
fixed at +-eps.
"""
import numpy as np
import pytest

import range_factored_cases as RF
import range_oracle as RO
import shared_cases as SC

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

EPS = 1e-6
SHAPES = [(5, 9, 2), (16, 32, 4), (20, 40, 4)]
FD_SHAPES = [(5, 9, 2), (20, 40, 4)]  # one shape of each kernel class
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


def _grads(qpb, H0, f, A0, bl, bu, meq, w, **kw):
    ins = [_dev(v, True) for v in (H0, f, A0, bl, bu)]
    x, status = qpb.diff.solve_range(*ins, meq, **kw)
    assert not status.requires_grad and (status == qpb.OK).all()
    (_dev(w) * x).sum().backward()
    torch.cuda.synchronize()
    return x.detach().cpu().numpy(), [t.grad.cpu().numpy() for t in ins]


@pytest.mark.parametrize("n,m,meq", SHAPES)
def test_prefactor_is_factor_solve_and_the_shared_backward(qpb, n, m, meq):
    H0, f, A0, bl, bu, _ = RF.family(B, n, m, meq)
    w = np.random.default_rng([SC.SEED, n, m]).standard_normal((B, n))
    x, grads = _grads(qpb, H0, f, A0, bl, bu, meq, w, prefactor=True)
    sol = qpb.solve_range_factored(qpb.factor_shared(_dev(H0), _dev(A0)), _dev(f), _dev(bl), _dev(bu), meq)
    gH, gf, gA, gb = qpb.solve_shared_backward(_dev(H0), _dev(A0),
                                               qpb.Solution(sol.x, sol.lam, sol.active, sol.status, None), _dev(w))
    torch.cuda.synchronize()
    assert np.array_equal(x, sol.x.cpu().numpy())
    low = RO.unpack_bits(sol.lower.cpu().numpy(), m)
    gb = gb.cpu().numpy()
    want = (gH.cpu().numpy(), gf.cpu().numpy(), gA.cpu().numpy(), np.where(low, gb, 0.0), np.where(low, 0.0, gb))
    for g, v, shape in zip(grads, want, ((n, n), (B, n), (m, n), (B, m), (B, m))):
        assert g.shape == shape and np.array_equal(g, v), shape
    assert low.any() and (grads[3] != 0).any() and (grads[4] != 0).any()
    assert (grads[3][:, :meq] == 0).all()


@pytest.mark.parametrize("n,m,meq", SHAPES)
def test_prefactor_against_the_default(qpb, n, m, meq):
    H0, f, A0, bl, bu, _ = RF.family(B, n, m, meq)
    assert RF.oracle(B, n, m, meq)[4].all()  # strictly complementary: one active set for both paths
    w = np.random.default_rng([SC.SEED, n, m, 1]).standard_normal((B, n))
    xf, gf = _grads(qpb, H0, f, A0, bl, bu, meq, w, prefactor=True)
    xd, gd = _grads(qpb, H0, f, A0, bl, bu, meq, w, prefactor=False)
    xn, gn = _grads(qpb, H0, f, A0, bl, bu, meq, w)
    assert np.array_equal(xd, xn) and all(np.array_equal(a, b) for a, b in zip(gd, gn))  # the default is the default
    rel = np.abs(xf - xd).max(axis=1) / np.maximum(1.0, np.abs(xd).max(axis=1))
    worst = [float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) for a, b in zip(gf, gd)]
    print(f"({n},{m},{meq}) B={B}: x {rel.max():.2e}; gradients for H, f, A, bl, bu {['%.2e' % v for v in worst]}")
    assert rel.max() <= RF.X_TOL
    assert np.array_equal(gf[3] != 0, gd[3] != 0) and np.array_equal(gf[4] != 0, gd[4] != 0)  # the same routing
    assert all(v <= 1e-6 for v in worst), worst
    assert gf[0].shape == (n, n) and gf[2].shape == (m, n)


@pytest.mark.parametrize("n,m,meq", FD_SHAPES)
def test_backward_matches_a_central_difference_of_the_factored_forward(qpb, n, m, meq):
    H0, f, A0, bl, bu, _ = RF.family(B, n, m, meq)
    x, lam, act, low, strict, _ = RF.oracle(B, n, m, meq)
    ax, ineq = x @ A0.T, np.arange(m) >= meq
    lam_min = np.where(act & ineq, np.abs(lam), np.inf).min()
    slack_min = min(np.where(~act & ineq, np.minimum(bu - ax, ax - bl), np.inf).min(),
                    np.where(act & ineq, np.where(low, bu - ax, ax - bl), np.inf).min())
    print(f"({n},{m},{meq}) B={B}: smallest active |lam| {lam_min:.3g}, smallest inactive slack {slack_min:.3g}")
    assert lam_min >= 160.0 and slack_min >= 0.03
    rng = np.random.default_rng([SC.SEED, n, m, 2])
    w = rng.standard_normal((B, n))
    dH = rng.standard_normal((n, n))
    dH = 0.5 * (dH + dH.T)
    df, dA = rng.standard_normal((B, n)), rng.standard_normal((m, n))
    dl, du = rng.standard_normal((B, m)), rng.standard_normal((B, m))
    _, grads = _grads(qpb, H0, f, A0, bl, bu, meq, w, prefactor=True)
    ana = sum(float((g * d).sum()) for g, d in zip(grads, (dH, df, dA, dl, du)))

    def value(s):
        F = qpb.factor_shared(_dev(H0 + s * dH), _dev(A0 + s * dA))
        sol = qpb.solve_range_factored(F, _dev(f + s * df), _dev(bl + s * dl), _dev(bu + s * du), meq)
        torch.cuda.synchronize()
        assert (sol.status == qpb.OK).all()
        return float((w * sol.x.cpu().numpy()).sum()), sol.active.cpu().numpy(), sol.lower.cpu().numpy()

    (lp, ap, wp), (lm, am, wm) = value(EPS), value(-EPS)
    num = (lp - lm) / (2 * EPS)
    rel = abs(ana - num) / (1.0 + abs(num))
    print(f"({n},{m},{meq}) B={B}: autograd {ana:.9e} central difference {num:.9e} relative {rel:.2e}")
    assert np.array_equal(ap, am) and np.array_equal(wp, wm)  # the same sets on both sides
    assert rel <= 1e-4
    assert (grads[3] != 0).any() and (grads[4] != 0).any()


def test_prefactor_needs_one_matrix_for_the_batch(qpb):
    n, m, meq = 16, 32, 4
    H0, f, A0, bl, bu, _ = RF.family(B, n, m, meq)
    with pytest.raises(ValueError):
        qpb.diff.solve_range(_dev(SC.expand(H0, B)), _dev(f), _dev(A0), _dev(bl), _dev(bu), meq, prefactor=True)
    with pytest.raises(ValueError):
        qpb.diff.solve_range(_dev(H0), _dev(f), _dev(SC.expand(A0, B)), _dev(bl), _dev(bu), meq, prefactor=True)
    # ... which the default takes
    x, status = qpb.diff.solve_range(_dev(SC.expand(H0, B)), _dev(f), _dev(A0), _dev(bl), _dev(bu), meq)
    assert (status == qpb.OK).all()
