"""qpb.diff.solve_range_box on the GPU: torch autograd through the solve with
two-sided rows beside variable bounds.

loss = (w . x).sum() through qpb.diff.solve_range_box; .backward() is compared
with the test's own central difference (EPS = 1e-6) of qpb.solve_range_box along
one seeded direction that moves all of H (symmetrised), f, G, bl, bu, lb and ub
at once.  The bar is 1e-4 relative, as in tests/test_gpu_range_autograd.py: on
these batches -- the 24 QPs per shape that tests/test_range_box_oracle.py pins --
every active |lam| is >= 1 and every inactive slack >= 1e-3 (re-asserted below),
which keeps `active` and `lower` fixed at +-EPS; the margin covers the noise of
a finite difference of fp64 solves.
"""
import numpy as np
import pytest

import range_box_oracle as BO
import range_oracle as RO

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

EPS = 1e-6
COUNT = 24
SHAPES = [(16, 16, 2), (12, 20, 0), (20, 9, 0)]  # n, mg, meq


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    import qpb.diff  # noqa: F401
    return q


def _dev(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda().requires_grad_(grad)


def _margins(n, mg, meq):
    (H, f, G, bl, bu, lb, ub, xc), (A, lo, hi), refs = BO.box_reference(COUNT, n, mg, meq)
    act = np.array([r.active for r in refs])
    lam = np.array([r.lam for r in refs])
    ax = np.einsum("bij,bj->bi", A, np.array([r.x for r in refs]))
    slack = np.minimum(hi - ax, ax - lo)
    return np.abs(lam[act]).min(), slack[~act & (np.arange(mg + n) >= meq)].min()


@pytest.mark.parametrize("n,mg,meq", SHAPES)
def test_backward_matches_a_central_difference(qpb, n, mg, meq):
    (H, f, G, bl, bu, lb, ub, _), _, _ = BO.box_reference(COUNT, n, mg, meq)
    lam_min, slack_min = _margins(n, mg, meq)
    print(f"({n},{mg},{meq}) B={COUNT}: smallest active |lam| {lam_min:.3g}, smallest inactive slack {slack_min:.3g}")
    assert lam_min >= 1.0 and slack_min >= 1e-3
    rng = np.random.default_rng([21, n, mg])
    w = rng.standard_normal((COUNT, n))
    dH = rng.standard_normal((COUNT, n, n))
    dH = 0.5 * (dH + dH.transpose(0, 2, 1))
    df, dG = rng.standard_normal((COUNT, n)), rng.standard_normal((COUNT, mg, n))
    dbl, dbu = rng.standard_normal((COUNT, mg)), rng.standard_normal((COUNT, mg))
    dlb, dub = rng.standard_normal((COUNT, n)), rng.standard_normal((COUNT, n))
    inputs = (H, f, G, bl, bu, lb, ub)
    dirs = (dH, df, dG, dbl, dbu, dlb, dub)
    leaves = [_dev(v, True) for v in inputs]
    x, status = qpb.diff.solve_range_box(*leaves, meq)
    assert not status.requires_grad and (status == qpb.OK).all()
    (_dev(w) * x).sum().backward()
    torch.cuda.synchronize()
    assert all(t.grad is not None and t.grad.shape == t.shape for t in leaves)
    parts = [float((t.grad.cpu().numpy() * d).sum()) for t, d in zip(leaves, dirs)]
    ana = sum(parts)

    def value(s, only=None):
        args = [_dev(v + s * d) if only is None or k == only else _dev(v)
                for k, (v, d) in enumerate(zip(inputs, dirs))]
        sol = qpb.solve_range_box(*args, meq)
        torch.cuda.synchronize()
        assert (sol.status == qpb.OK).all()
        return float((w * sol.x.cpu().numpy()).sum()), sol.active.cpu().numpy(), sol.lower.cpu().numpy()

    (lp, ap, wp), (lm, am, wm) = value(EPS), value(-EPS)
    num = (lp - lm) / (2 * EPS)
    rel = abs(ana - num) / (1.0 + abs(num))
    print(f"({n},{mg},{meq}) B={COUNT}: autograd {ana:.9e} central difference {num:.9e} relative {rel:.2e}")
    assert np.array_equal(ap, am) and np.array_equal(wp, wm)  # the same sets on both sides
    assert rel <= 1e-4
    # ... and for every input on its own
    for k, name in enumerate(("H", "f", "G", "bl", "bu", "lb", "ub")):
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
def test_gb_is_routed_by_the_lower_bits(qpb, n, mg, meq):
    (H, f, G, bl, bu, lb, ub, _), (A, lo, hi), _ = BO.box_reference(COUNT, n, mg, meq)
    m = mg + n
    Hd, fd, Gd = _dev(H), _dev(f), _dev(G)
    blt, but, lbt, ubt = (_dev(v, True) for v in (bl, bu, lb, ub))
    x, _ = qpb.diff.solve_range_box(Hd, fd, Gd, blt, but, lbt, ubt, meq)
    w = _dev(np.random.default_rng([22, n, mg]).standard_normal((COUNT, n)))
    (w * x).sum().backward()
    sol = qpb.solve_range_box(Hd, fd, Gd, _dev(bl), _dev(bu), _dev(lb), _dev(ub), meq)
    _, _, _, gb = qpb.solve_backward(Hd, _dev(A), qpb.Solution(sol.x, sol.lam, sol.active, sol.status, None), w,
                                     need=("b",))
    torch.cuda.synchronize()
    low = RO.unpack_bits(sol.lower.cpu().numpy(), m)
    gb = gb.cpu().numpy()
    glo = np.concatenate([blt.grad.cpu().numpy(), lbt.grad.cpu().numpy()], axis=1)
    ghi = np.concatenate([but.grad.cpu().numpy(), ubt.grad.cpu().numpy()], axis=1)
    assert np.array_equal(glo + ghi, gb)  # one of the two is an exact 0 everywhere
    assert np.array_equal(np.where(low, gb, 0.0), glo) and np.array_equal(np.where(low, 0.0, gb), ghi)
    assert (glo[:, :meq] == 0).all()
    # the variables' part lands in lb against ub by the bits mg + j
    assert low[:, mg:].any() and (lbt.grad != 0).any() and (ubt.grad != 0).any()
    assert (lbt.grad.cpu().numpy()[~low[:, mg:]] == 0).all() and (ubt.grad.cpu().numpy()[low[:, mg:]] == 0).all()


def test_a_shared_G_gets_one_summed_gradient(qpb):
    n, mg, meq = 16, 16, 2
    (H, f, G, bl, bu, lb, ub, xc), _, _ = BO.box_reference(COUNT, n, mg, meq)
    G0 = G[0]
    gx = np.einsum("ij,bj->bi", G0, xc)
    rng = np.random.default_rng([23, n, mg])
    buS = gx + rng.uniform(0.05, 1.0, size=gx.shape)
    blS = gx - rng.uniform(0.05, 1.0, size=gx.shape)
    blS[:, :meq] = buS[:, :meq] = gx[:, :meq]
    Hd, fd, Gt = _dev(H), _dev(f), _dev(G0, True)
    w = _dev(rng.standard_normal((COUNT, n)))
    x, status = qpb.diff.solve_range_box(Hd, fd, Gt, _dev(blS), _dev(buS), _dev(lb), _dev(ub), meq)
    assert (status == qpb.OK).all()
    (w * x).sum().backward()
    sol = qpb.solve_range_box(Hd, fd, _dev(G0), _dev(blS), _dev(buS), _dev(lb), _dev(ub), meq)
    A0 = _dev(np.concatenate([G0, np.eye(n)], axis=0))
    _, _, gA, _ = qpb.solve_shared_backward(Hd, A0, qpb.Solution(sol.x, sol.lam, sol.active, sol.status, None), w,
                                            need=("A",))
    torch.cuda.synchronize()
    assert tuple(Gt.grad.shape) == (mg, n) and tuple(gA.shape) == (mg + n, n)
    assert torch.equal(Gt.grad, gA[:mg]) and bool((Gt.grad != 0).any())


def test_a_bound_passed_as_none_gets_no_gradient(qpb):
    n, mg, meq = 12, 20, 0
    (H, f, G, bl, bu, lb, ub, _), _, _ = BO.box_reference(COUNT, n, mg, meq)
    names = ("bl", "bu", "lb", "ub")
    for which in names:
        ft = _dev(f, True)
        leaves = {k: _dev(v, True) for k, v in zip(names, (bl, bu, lb, ub))}
        args = [None if k == which else leaves[k] for k in names]
        x, status = qpb.diff.solve_range_box(_dev(H), ft, _dev(G), *args, meq)
        assert (status == qpb.OK).all()
        x.sum().backward()
        torch.cuda.synchronize()
        assert ft.grad is not None
        for k in names:
            assert (leaves[k].grad is None) == (k == which), (which, k)
    # a bound that does not require grad gets none either, and G = None has no gradient to give
    lbt, ubt = _dev(lb), _dev(ub, True)
    x, _ = qpb.diff.solve_range_box(_dev(H), _dev(f), None, None, None, lbt, ubt)
    x.sum().backward()
    assert lbt.grad is None and ubt.grad is not None and tuple(ubt.grad.shape) == (COUNT, n)


def test_forward_raises_above_the_limit(qpb):
    n, Bq = 33, 2
    H = np.broadcast_to(np.eye(n), (Bq, n, n)).copy()
    with pytest.raises(qpb.QPBError) as e:
        qpb.diff.solve_range_box(_dev(H), _dev(np.ones((Bq, n)), True), None, None, None, _dev(-np.ones((Bq, n))),
                                 _dev(np.ones((Bq, n))))
    assert e.value.code == qpb.ERR_UNSUPPORTED
