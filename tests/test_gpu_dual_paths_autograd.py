"""The Python layer over qpb_solve_factored_backward_dual and
qpb_solve_box_backward_dual on the GPU: qpb.solve_factored_tangent and
qpb.solve_box_tangent, qpb.diff.solve_dual / solve_range_dual with
prefactor=True, and qpb.diff.solve_box_dual.

Tangents and autograd gradients are compared with the test's own central
difference (eps = 1e-6) of the GPU forward; the bar is 1e-4 relative, the
constants of tests/test_gpu_tangent.py and tests/test_gpu_dual_autograd.py: the
active set stays fixed at +-eps (asserted), the margin covers the noise of a
finite difference of fp64 solves.  The box family is box_bwd_oracle.family at
width 10, which tests/test_box_bwd_oracle.py shows to be safe for such a step.
Where a backward contract is bit for bit, so is the comparison: the factored
calls against the unfactored ones on the same forward outputs, one H against
copies of it, a loss in x alone against solve_box's gradients.  A prefactored
forward's x and lam are held to the unfactored one's within 1e-6 relative, the
factored tests' rounding bar.
"""
import numpy as np
import pytest

import box_bwd_oracle as BO
import shared_cases as SC

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

EPS = 1e-6
FD_TOL = 1e-4
X_TOL = 1e-6
SEED = 11
B = 8
SHAPES = [(5, 9, 2), (16, 32, 4), (20, 40, 4)]
BOX_SHAPES = [5, 16, 20]


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    import qpb.diff  # noqa: F401
    return q


def _dev(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda().requires_grad_(grad)


def _eq(a, c):
    return np.array_equal(a.detach().cpu().numpy().view(np.uint8), c.detach().cpu().numpy().view(np.uint8))


def _rel(a, ref):
    return np.abs(a - ref).max() / (1.0 + np.abs(ref).max())


class Called(Exception):
    pass


def _raise(*a, **kw):
    raise Called("the unfactored backward")


# ------------------------------------------------------- tangents
@pytest.mark.parametrize("n,m,meq", SHAPES)
def test_factored_tangent(qpb, n, m, meq):
    H0, f, A0, b = SC.family(B, n, m, meq)
    rng = np.random.default_rng([SEED, n, m, 23])
    df, db = rng.standard_normal((B, n)), rng.standard_normal((B, m))
    Hd, Ad = _dev(H0), _dev(A0)
    fwd = qpb.factor_shared(Hd, Ad)
    sol = qpb.solve_factored(fwd, _dev(f), _dev(b), meq)
    F = qpb.factor_shared_backward(Hd, Ad)
    dx, dlam = qpb.solve_factored_tangent(F, sol, _dev(df), _dev(db))
    want = qpb.solve_tangent(Hd, Ad, sol, _dev(df), _dev(db))
    torch.cuda.synchronize()
    assert (sol.status == qpb.OK).all()
    assert _eq(dx, want[0]) and _eq(dlam, want[1])  # bit for bit the unfactored tangent
    mask = qpb.active_mask_to_bool(sol.active.cpu().numpy(), m)
    dx, dlam = dx.cpu().numpy(), dlam.cpu().numpy()
    assert (dlam[~mask] == 0.0).all()

    def side(s):
        p = qpb.solve_factored(fwd, _dev(f + s * df), _dev(b + s * db), meq)
        torch.cuda.synchronize()
        assert (p.status == qpb.OK).all() and torch.equal(p.active, sol.active)  # the same active set
        return p.x.cpu().numpy(), p.lam.cpu().numpy()

    (xp, lp), (xm, lm) = side(EPS), side(-EPS)
    ex, el = _rel(dx, (xp - xm) / (2 * EPS)), _rel(dlam, (lp - lm) / (2 * EPS))
    print(f"({n},{m},{meq}): |tangent - central difference| / (1 + |cd|): x {ex:.2e} lam {el:.2e}")
    assert ex <= FD_TOL and el <= FD_TOL
    # db = None takes qpb_solve_factored_backward's kernels
    dx0, dl0 = qpb.solve_factored_tangent(F, sol, _dev(df))
    _, gf, _, gb = qpb.solve_factored_backward(F, sol, _dev(df), need=("f", "b"))
    torch.cuda.synchronize()
    assert _eq(dx0, gf) and _eq(dl0, -gb)


@pytest.mark.parametrize("n", BOX_SHAPES)
def test_box_tangent(qpb, n):
    H, f, lb, ub = BO.family(SEED, B, n, 10.0)
    rng = np.random.default_rng([SEED, n, 24])
    df, dlb, dub = (rng.standard_normal((B, n)) for _ in range(3))
    Hd = _dev(H)
    sol = qpb.solve_box(Hd, _dev(f), _dev(lb), _dev(ub))
    dx, dlam = qpb.solve_box_tangent(Hd, sol, _dev(df), _dev(dlb), _dev(dub))
    torch.cuda.synchronize()
    assert (sol.status == qpb.OK).all() and tuple(dlam.shape) == (B, 2 * n)
    mask = qpb.active_mask_to_bool(sol.active.cpu().numpy(), 2 * n)
    assert mask.any() and not mask.all()
    dxn, dln = dx.cpu().numpy(), dlam.cpu().numpy()
    assert (dln[~mask] == 0.0).all()
    # a fixed variable moves with its bound, exactly
    assert np.array_equal(dxn[mask[:, :n]], dub[mask[:, :n]]) and np.array_equal(dxn[mask[:, n:]], dlb[mask[:, n:]])

    def side(s):
        p = qpb.solve_box(Hd, _dev(f + s * df), _dev(lb + s * dlb), _dev(ub + s * dub))
        torch.cuda.synchronize()
        assert (p.status == qpb.OK).all() and torch.equal(p.active, sol.active)  # the same active set
        return p.x.cpu().numpy(), p.lam.cpu().numpy()

    (xp, lp), (xm, lm) = side(EPS), side(-EPS)
    ex, el = _rel(dxn, (xp - xm) / (2 * EPS)), _rel(dln, (lp - lm) / (2 * EPS))
    print(f"n={n}: |tangent - central difference| / (1 + |cd|): x {ex:.2e} lam {el:.2e}")
    assert ex <= FD_TOL and el <= FD_TOL
    # one H for the batch: bit for bit the call on copies of it
    H0 = _dev(H[0])
    copies = _dev(SC.expand(H[0], B))
    one = qpb.solve_box_tangent(H0, sol, _dev(df), _dev(dlb), _dev(dub))
    ref = qpb.solve_box_tangent(copies, sol, _dev(df), _dev(dlb), _dev(dub))
    # the bounds at rest: the box backward's kernels
    rest = qpb.solve_box_tangent(Hd, sol, _dev(df))
    _, gf, glb, gub = qpb.solve_box_backward(Hd, sol, _dev(df), need=("f", "lb", "ub"))
    torch.cuda.synchronize()
    assert _eq(one[0], ref[0]) and _eq(one[1], ref[1])
    assert _eq(rest[0], gf) and _eq(rest[1], torch.cat((-gub, glb), dim=1))


# ------------------------------------------------------- solve_dual / solve_range_dual with prefactor
@pytest.mark.parametrize("n,m,meq", SHAPES)
def test_solve_dual_prefactor(qpb, monkeypatch, n, m, meq):
    H0, f, A0, b = SC.family(B, n, m, meq)
    rng = np.random.default_rng([SEED, n, m, 25])
    w, v = rng.standard_normal((B, n)), rng.standard_normal((B, m))
    sol = qpb.solve_factored(qpb.factor_shared(_dev(H0), _dev(A0)), _dev(f), _dev(b), meq)
    want = qpb.solve_backward_dual(_dev(H0), _dev(A0), sol, _dev(w), _dev(v))
    want_x = qpb.solve_shared_backward(_dev(H0), _dev(A0), sol, _dev(w))
    plain = qpb.solve_shared(_dev(H0), _dev(f), _dev(A0), _dev(b), meq)
    torch.cuda.synchronize()
    monkeypatch.setattr(qpb, "solve_backward_dual", _raise)
    monkeypatch.setattr(qpb, "solve_shared_backward", _raise)
    ins = [_dev(t, True) for t in (H0, f, A0, b)]
    x, lam, status = qpb.diff.solve_dual(*ins, meq, prefactor=True)
    assert (status == qpb.OK).all() and not status.requires_grad and lam.requires_grad
    assert _eq(x, sol.x) and _eq(lam, sol.lam)
    # the forward against the unfactored one: by rounding
    assert _rel(x.detach().cpu().numpy(), plain.x.cpu().numpy()) <= X_TOL
    assert _rel(lam.detach().cpu().numpy(), plain.lam.cpu().numpy()) <= X_TOL
    ((_dev(w) * x).sum() + (_dev(v) * lam).sum()).backward()
    torch.cuda.synchronize()
    for t, g, shape in zip(ins, want, ((n, n), (B, n), (m, n), (B, m))):
        assert tuple(t.grad.shape) == shape and _eq(t.grad, g), shape
    # a loss that does not read lam takes the factored backward without glam
    ins = [_dev(t, True) for t in (H0, f, A0, b)]
    x, lam, _ = qpb.diff.solve_dual(*ins, meq, prefactor=True)
    (_dev(w) * x).sum().backward()
    torch.cuda.synchronize()
    for t, g in zip(ins, want_x):
        assert _eq(t.grad, g)
    # the default is the patched call
    ins = [_dev(t, True) for t in (H0, f, A0, b)]
    x, lam, _ = qpb.diff.solve_dual(*ins, meq)
    with pytest.raises(Called):
        ((_dev(w) * x).sum() + (_dev(v) * lam).sum()).backward()


@pytest.mark.parametrize("n,m,meq", SHAPES)
def test_solve_range_dual_prefactor(qpb, monkeypatch, n, m, meq):
    H0, f, A0, b = SC.family(B, n, m, meq)
    bl = b - np.random.default_rng([SC.SEED, n, m, 18]).uniform(10.0, 50.0, size=b.shape)  # at least the family's slack
    rng = np.random.default_rng([SEED, n, m, 26])
    w, v = rng.standard_normal((B, n)), rng.standard_normal((B, m))
    sol = qpb.solve_range_factored(qpb.factor_shared(_dev(H0), _dev(A0)), _dev(f), _dev(bl), _dev(b), meq)
    bsol = qpb.Solution(sol.x, sol.lam, sol.active, sol.status, None)
    gH, gf, gA, gb = qpb.solve_backward_dual(_dev(H0), _dev(A0), bsol, _dev(w), _dev(v))
    plain = qpb.solve_range(_dev(H0), _dev(f), _dev(A0), _dev(bl), _dev(b), meq)
    torch.cuda.synchronize()
    monkeypatch.setattr(qpb, "solve_backward_dual", _raise)
    ins = [_dev(t, True) for t in (H0, f, A0, bl, b)]
    x, lam, status = qpb.diff.solve_range_dual(*ins, meq, prefactor=True)
    assert (status == qpb.OK).all() and _eq(x, sol.x) and _eq(lam, sol.lam)
    assert _rel(x.detach().cpu().numpy(), plain.x.cpu().numpy()) <= X_TOL
    assert _rel(lam.detach().cpu().numpy(), plain.lam.cpu().numpy()) <= X_TOL
    ((_dev(w) * x).sum() + (_dev(v) * lam).sum()).backward()
    torch.cuda.synchronize()
    Ht, ft, At, blt, but = ins
    assert tuple(Ht.grad.shape) == (n, n) and _eq(Ht.grad, gH) and _eq(ft.grad, gf) and _eq(At.grad, gA)
    # gb goes to bl where the row's `lower` bit is set, to bu elsewhere
    low = qpb.active_mask_to_bool(sol.lower.cpu().numpy(), m)
    gbn = gb.cpu().numpy()
    assert np.array_equal(blt.grad.cpu().numpy().view(np.uint8), np.where(low, gbn, 0.0).view(np.uint8))
    assert np.array_equal(but.grad.cpu().numpy().view(np.uint8), np.where(low, 0.0, gbn).view(np.uint8))
    ins = [_dev(t, True) for t in (H0, f, A0, bl, b)]
    x, lam, _ = qpb.diff.solve_range_dual(*ins, meq)
    with pytest.raises(Called):
        ((_dev(w) * x).sum() + (_dev(v) * lam).sum()).backward()


# ------------------------------------------------------- solve_box_dual
@pytest.mark.parametrize("n", BOX_SHAPES)
@pytest.mark.parametrize("form", ["3-D H", "2-D H", "2-D H, prefactor"])
def test_solve_box_dual_matches_a_central_difference(qpb, n, form):
    """loss = (w . x).sum() + (v . lam).sum() along one seeded direction that moves H (symmetrised), f, lb and ub at once."""
    Bq = 4
    H, f, lb, ub = BO.family(SEED, Bq, n, 10.0)
    shared = form != "3-D H"
    kw = {"prefactor": True} if form.endswith("prefactor") else {}
    if shared:
        H = H[0]
    rng = np.random.default_rng([SEED, n, 27])
    w, v = rng.standard_normal((Bq, n)), rng.standard_normal((Bq, 2 * n))
    dH = rng.standard_normal(H.shape)
    dH = 0.5 * (dH + np.swapaxes(dH, -1, -2))
    df, dl, du = (rng.standard_normal((Bq, n)) for _ in range(3))
    ins = [_dev(t, True) for t in (H, f, lb, ub)]
    x, lam, status = qpb.diff.solve_box_dual(*ins, **kw)
    assert not status.requires_grad and (status == qpb.OK).all() and lam.requires_grad and tuple(lam.shape) == (Bq, 2 * n)
    ((_dev(w) * x).sum() + (_dev(v) * lam).sum()).backward()
    torch.cuda.synchronize()
    assert tuple(ins[0].grad.shape) == H.shape
    ana = sum(float((t.grad.cpu().numpy() * d).sum()) for t, d in zip(ins, (dH, df, dl, du)))
    forward = qpb.solve_box_shared if shared else qpb.solve_box

    def value(s):
        sol = forward(_dev(H + s * dH), _dev(f + s * df), _dev(lb + s * dl), _dev(ub + s * du))
        torch.cuda.synchronize()
        assert (sol.status == qpb.OK).all()
        return float((w * sol.x.cpu().numpy()).sum() + (v * sol.lam.cpu().numpy()).sum()), sol.active.cpu().numpy()

    (lp, ap), (lm, am) = value(EPS), value(-EPS)
    num = (lp - lm) / (2 * EPS)
    rel = abs(ana - num) / (1.0 + abs(num))
    print(f"n={n} {form}: autograd {ana:.9e} central difference {num:.9e} relative {rel:.2e}")
    assert np.array_equal(ap, am)  # the same active set on both sides
    assert rel <= FD_TOL
    g = ins[0].grad.cpu().numpy()
    assert np.array_equal(g, np.swapaxes(g, -1, -2))


@pytest.mark.parametrize("n", [5, 20])
@pytest.mark.parametrize("shared", [False, True])
def test_a_loss_in_x_alone_gives_solve_boxs_gradients_bit_for_bit(qpb, n, shared):
    Bq = 4
    H, f, lb, ub = BO.family(SEED, Bq, n, 10.0)
    if shared:
        H = H[0]
    w = _dev(np.random.default_rng([SEED, n, 28]).standard_normal((Bq, n)))
    one = [_dev(t, True) for t in (H, f, lb, ub)]
    x, status = qpb.diff.solve_box(*one)
    (w * x).sum().backward()
    two = [_dev(t, True) for t in (H, f, lb, ub)]
    x2, lam2, _ = qpb.diff.solve_box_dual(*two)
    (w * x2).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(x, x2)
    for a, c in zip(one, two):
        assert _eq(a.grad, c.grad)
    # a loss in lam alone: gx = 0
    three = [_dev(t, True) for t in (H, f, lb, ub)]
    x3, lam3, _ = qpb.diff.solve_box_dual(*three)
    v = _dev(np.random.default_rng([SEED, n, 29]).standard_normal((Bq, 2 * n)))
    (v * lam3).sum().backward()
    sol = qpb.Solution(x3.detach(), None, (qpb.solve_box_shared if shared else qpb.solve_box)(
        _dev(H), _dev(f), _dev(lb), _dev(ub)).active, None, None)
    want = qpb.solve_box_backward_dual(_dev(H), sol, torch.zeros_like(w), v)
    torch.cuda.synchronize()
    for a, g in zip(three, want):
        assert _eq(a.grad, g)
