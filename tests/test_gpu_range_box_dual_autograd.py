"""qpb.diff.solve_range_box_dual on the GPU: torch autograd through the solve
with two-sided rows beside variable bounds, for a loss that reads x AND lam.

loss = (w . x).sum() + (v . lam).sum() through qpb.diff.solve_range_box_dual;
.backward() is compared with the test's own central difference (EPS = 1e-6) of
qpb.solve_range_box along one seeded direction that moves all of H
(symmetrised), f, G, bl, bu, lb and ub at once, and along each input alone.
EPS, the bar of 1e-4 relative and the three shapes are those of
tests/test_gpu_range_box_autograd.py: on these batches every active |lam| is
>= 1 and every inactive slack >= 1e-3 (tests/test_range_box_bwd_cases.py), which
keeps `active` and `lower` fixed at +-EPS; lam is zero outside the active set on
both sides of the difference.
"""
import numpy as np
import pytest

import range_box_oracle as BO

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

EPS = 1e-6
COUNT = 24
SHAPES = [(16, 16, 2), (12, 20, 0), (20, 9, 0)]  # n, mg, meq
NAMES = ("H", "f", "G", "bl", "bu", "lb", "ub")


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    import qpb.diff  # noqa: F401
    return q


def _dev(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda().requires_grad_(grad)


@pytest.mark.parametrize("n,mg,meq", SHAPES)
def test_backward_matches_a_central_difference(qpb, n, mg, meq):
    (H, f, G, bl, bu, lb, ub, _), _, _ = BO.box_reference(COUNT, n, mg, meq)
    rng = np.random.default_rng([41, n, mg])
    w, v = rng.standard_normal((COUNT, n)), rng.standard_normal((COUNT, mg + n))
    dH = rng.standard_normal((COUNT, n, n))
    dH = 0.5 * (dH + dH.transpose(0, 2, 1))
    df, dG = rng.standard_normal((COUNT, n)), rng.standard_normal((COUNT, mg, n))
    dbl, dbu = rng.standard_normal((COUNT, mg)), rng.standard_normal((COUNT, mg))
    dlb, dub = rng.standard_normal((COUNT, n)), rng.standard_normal((COUNT, n))
    inputs = (H, f, G, bl, bu, lb, ub)
    dirs = (dH, df, dG, dbl, dbu, dlb, dub)
    leaves = [_dev(t, True) for t in inputs]
    x, lam, status = qpb.diff.solve_range_box_dual(*leaves, meq)
    assert not status.requires_grad and (status == qpb.OK).all()
    assert tuple(lam.shape) == (COUNT, mg + n) and lam.requires_grad
    ((_dev(w) * x).sum() + (_dev(v) * lam).sum()).backward()
    torch.cuda.synchronize()
    assert all(t.grad is not None and t.grad.shape == t.shape for t in leaves)
    parts = [float((t.grad.cpu().numpy() * d).sum()) for t, d in zip(leaves, dirs)]
    ana = sum(parts)

    def value(s, only=None):
        args = [_dev(t + s * d) if only is None or k == only else _dev(t)
                for k, (t, d) in enumerate(zip(inputs, dirs))]
        sol = qpb.solve_range_box(*args, meq)
        torch.cuda.synchronize()
        assert (sol.status == qpb.OK).all()
        loss = float((w * sol.x.cpu().numpy()).sum() + (v * sol.lam.cpu().numpy()).sum())
        return loss, sol.active.cpu().numpy(), sol.lower.cpu().numpy()

    (lp, ap, wp), (lm, am, wm) = value(EPS), value(-EPS)
    num = (lp - lm) / (2 * EPS)
    rel = abs(ana - num) / (1.0 + abs(num))
    print(f"({n},{mg},{meq}) B={COUNT}: autograd {ana:.9e} central difference {num:.9e} relative {rel:.2e}")
    assert np.array_equal(ap, am) and np.array_equal(wp, wm)  # the same sets on both sides
    assert rel <= 1e-4
    # ... and for every input on its own
    for k, name in enumerate(NAMES):
        (lp, ap, wp), (lm, am, wm) = value(EPS, k), value(-EPS, k)
        num_k = (lp - lm) / (2 * EPS)
        rel_k = abs(parts[k] - num_k) / (1.0 + abs(num_k))
        print(f"    {name}: autograd {parts[k]:.9e} central difference {num_k:.9e} relative {rel_k:.2e}")
        assert np.array_equal(ap, am) and np.array_equal(wp, wm)
        assert rel_k <= 1e-4, name
    Hg = leaves[0].grad.cpu().numpy()
    assert np.array_equal(Hg, Hg.transpose(0, 2, 1))
    assert all(bool((t.grad != 0).any()) for t in leaves)


@pytest.mark.parametrize("n,mg,meq", SHAPES)
def test_a_loss_that_ignores_lam_gets_solve_range_boxs_gradients(qpb, n, mg, meq):
    (H, f, G, bl, bu, lb, ub, _), _, _ = BO.box_reference(COUNT, n, mg, meq)
    w = _dev(np.random.default_rng([42, n, mg]).standard_normal((COUNT, n)))
    inputs = (H, f, G, bl, bu, lb, ub)
    plain = [_dev(t, True) for t in inputs]
    x, _ = qpb.diff.solve_range_box(*plain, meq)
    (w * x).sum().backward()
    dual = [_dev(t, True) for t in inputs]
    x2, lam, _ = qpb.diff.solve_range_box_dual(*dual, meq)
    assert torch.equal(x, x2)
    (w * x2).sum().backward()
    torch.cuda.synchronize()
    for name, a, b in zip(NAMES, plain, dual):
        assert np.array_equal(a.grad.cpu().numpy().view(np.int64), b.grad.cpu().numpy().view(np.int64)), name
    # a loss that reads lam alone has gx = 0, and moves every input
    only = [_dev(t, True) for t in inputs]
    _, lam, _ = qpb.diff.solve_range_box_dual(*only, meq)
    (lam * lam).sum().backward()
    torch.cuda.synchronize()
    assert all(t.grad is not None and bool((t.grad != 0).any()) for t in only)


def test_a_shared_H_and_G_get_one_summed_gradient_each(qpb):
    n, mg, meq = 16, 16, 2
    (H, f, G, bl, bu, lb, ub, xc), _, _ = BO.box_reference(COUNT, n, mg, meq)
    G0 = G[0]
    gxc = np.einsum("ij,bj->bi", G0, xc)
    rng = np.random.default_rng([43, n, mg])
    buS = gxc + rng.uniform(0.05, 1.0, size=gxc.shape)
    blS = gxc - rng.uniform(0.05, 1.0, size=gxc.shape)
    blS[:, :meq] = buS[:, :meq] = gxc[:, :meq]
    Ht, Gt = _dev(H[0], True), _dev(G0, True)
    x, lam, status = qpb.diff.solve_range_box_dual(Ht, _dev(f), Gt, _dev(blS), _dev(buS), _dev(lb), _dev(ub), meq)
    assert (status == qpb.OK).all()
    w, v = _dev(rng.standard_normal((COUNT, n))), _dev(rng.standard_normal((COUNT, mg + n)))
    ((w * x).sum() + (v * lam).sum()).backward()
    sol = qpb.solve_range_box(_dev(H[0]), _dev(f), _dev(G0), _dev(blS), _dev(buS), _dev(lb), _dev(ub), meq)
    A0 = _dev(np.concatenate([G0, np.eye(n)], axis=0))
    gH, _, gA, _ = qpb.solve_backward_dual(_dev(H[0]), A0, qpb.Solution(sol.x, sol.lam, sol.active, sol.status, None),
                                           w, v, need=("H", "A"))
    torch.cuda.synchronize()
    assert tuple(Ht.grad.shape) == (n, n) and tuple(Gt.grad.shape) == (mg, n)
    assert torch.equal(Ht.grad, gH) and torch.equal(Gt.grad, gA[:mg]) and bool((Gt.grad != 0).any())
