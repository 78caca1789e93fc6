"""qpb.diff.solve_box(H2d, f, lb, ub, prefactor=True) -- the forward on an H
factored once (qpb.factor_box + qpb.solve_box_factored), the backward
qpb.solve_box_shared_backward on the saved H, unchanged -- against the same
call with prefactor=False, at n = 5 and 20, B = 5.

The bars are the ones tests/test_gpu_box_shared_autograd.py holds the default
path to, carried over the one thing that differs, x by rounding (<= 1e-6
relative, tests/test_gpu_box.py's bar):
  status, and f.grad, lb.grad, ub.grad   bit for bit: the backward reads the
                active set, H and gx for them, never x, and the active sets are
                equal on this strictly complementary family.
  H.grad        (n, n), symmetric bit for bit; it is 1/2 sum_k (dx_k x_k^T +
                x_k dx_k^T) with the same dx_k, so the two differ by at most
                1/2 sum_k (|dx_k| |e_k|^T + |e_k| |dx_k|^T), |e_k| <= 1e-6
                max(1, |x_k|_inf), plus the summation bound of
                tests/shared_cases.py (sum_bound) that the default path is held
                to.
A 3-D H with prefactor=True raises ValueError; n = 33 raises
QPBError(ERR_UNSUPPORTED).
"""
import numpy as np
import pytest

import box_factored_cases as C
import box_shared_harness as BH
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


def _eq(a, c):
    return np.array_equal(a.detach().cpu().numpy().view(np.uint8), c.detach().cpu().numpy().view(np.uint8))


@pytest.mark.parametrize("n", [5, 20])
def test_prefactor_against_the_default_path(qpb, n):
    B = 5
    H0, f, lb, ub = BH.family(B, n)
    assert C.oracle(B, n)[3].all()  # every QP strictly complementary: a condition on the inputs
    w = _dev(np.random.default_rng([BH.SEED, n]).standard_normal((B, n)))
    Hp, fp, lp, up = (_dev(a).requires_grad_(True) for a in (H0, f, lb, ub))
    xp, stp = qpb.diff.solve_box(Hp, fp, lp, up, prefactor=True)
    (w * xp).sum().backward()
    Hd, fd, ld, ud = (_dev(a).requires_grad_(True) for a in (H0, f, lb, ub))
    xd, std = qpb.diff.solve_box(Hd, fd, ld, ud)
    (w * xd).sum().backward()
    torch.cuda.synchronize()
    assert (stp.cpu().numpy() == 0).all() and not stp.requires_grad and _eq(stp, std)
    x, xr = xp.detach().cpu().numpy(), xd.detach().cpu().numpy()
    print(f"n={n}: worst relative x difference {C.relx(x, xr).max():.3g}")
    assert C.relx(x, xr).max() <= C.X_TOL
    assert Hp.grad.shape == (n, n) and Hd.grad.shape == (n, n)
    assert _eq(fp.grad, fd.grad) and _eq(lp.grad, ld.grad) and _eq(up.grad, ud.grad)
    assert bool((lp.grad != 0).any()) and bool((up.grad != 0).any())  # both bounds' gradients take part
    g, gr = Hp.grad.cpu().numpy(), Hd.grad.cpu().numpy()
    assert np.array_equal(g.view(np.uint8), np.ascontiguousarray(g.T).view(np.uint8))
    dx = np.abs(fd.grad.cpu().numpy())
    e = C.X_TOL * np.maximum(1.0, np.abs(xr).max(axis=1))[:, None] * np.ones((B, n))
    moved = 0.5 * (np.einsum("ki,kj->ij", dx, e) + np.einsum("ki,kj->ij", e, dx))
    none = np.zeros((B, 0))
    bound = SC.sum_bound(xr, fd.grad.cpu().numpy(), none, none, np.zeros((B, 0), bool), np.ones(B, bool))[0]
    delta = np.abs(g - gr)
    print(f"n={n}: worst |delta| of H.grad {delta.max():.3g}, bound there "
          f"{(moved + 2 * bound).ravel()[delta.argmax()]:.3g}")
    assert (delta <= moved + 2 * bound).all()


def test_three_d_h_with_prefactor_raises(qpb):
    n, B = 5, 5
    H0, f, lb, ub = BH.family(B, n)
    with pytest.raises(ValueError):
        qpb.diff.solve_box(_dev(SC.expand(H0, B)), _dev(f), _dev(lb), _dev(ub), prefactor=True)


def test_n_33_is_unsupported(qpb):
    n, B = 33, 5
    H0, f, lb, ub = BH.family(B, n)
    with pytest.raises(qpb.QPBError) as e:
        qpb.diff.solve_box(_dev(H0), _dev(f), _dev(lb), _dev(ub), prefactor=True)
    assert e.value.code == qpb.ERR_UNSUPPORTED
