"""qpb_solve_box_shared on the GPU: one H for a batch of box QPs, read from one
copy.  The contract is equality bit for bit: x, lam, active, status and iters
of every QP are what qpb_solve_box writes for it on shared_cases.expand(H0, B)
-- on the feasible family of tests/box_shared_harness.py at every kernel class
(box-dense n in {1, 5, 16}: both N16 forms; wave n in {17, 20, 32}; Gram n in
{33, 128}), and with absent, infinite, NaN, pinned and crossed bounds, capped
iterations, NaN in f, a non-SPD and a NaN H0.  Every call goes through the
C-ABI into buffers filled with 0xA5 and fenced by guard words: every element is
written, nothing outside, and H0's device buffer is unchanged.
"""
import numpy as np
import pytest

import box_shared_harness as BH
import shared_cases as SC

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

OK, NOT_SPD = 0, 2
SHAPES = BH.DENSE_N + BH.WAVE_N + BH.GRAM_N
EDGE_SHAPES = (5, 16, 20, 33)  # one of each form below n = 128, at B = 67
EDGE_B = 67


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    return q


_REF = {}


def _reference(qpb, B, n):
    """qpb_solve_box on materialised copies: once per case, shared, never modified."""
    if (B, n) not in _REF:
        H0, f, lb, ub = BH.family(B, n)
        _REF[(B, n)] = BH.solve(qpb, SC.expand(H0, B), f, lb, ub)
    return _REF[(B, n)]


def _both(qpb, H0, f, lb, ub, **kw):
    """(shared, on copies) for one set of inputs."""
    B = f.shape[0]
    return BH.solve(qpb, H0, f, lb, ub, **kw), BH.solve(qpb, SC.expand(H0, B), f, lb, ub, **kw)


@pytest.mark.parametrize("n", SHAPES)
def test_bitwise_equal_to_solve_box_on_copies(qpb, n):
    for B in BH.batches_of(qpb, n):
        H0, f, lb, ub = BH.family(B, n)
        ref = _reference(qpb, B, n)
        assert (ref["status"] == OK).all(), (B, ref["status"])  # lb < 0 < ub: every QP is feasible
        got = BH.solve(qpb, H0, f, lb, ub)
        assert BH.same(got, ref), B


@pytest.mark.parametrize("n", EDGE_SHAPES + (128,))
def test_absent_bounds(qpb, n):
    B = 5 if n == 128 else EDGE_B
    H0, f, lb, ub = BH.family(B, n)
    for lo, up in ((None, ub), (lb, None), (None, None)):
        got, ref = _both(qpb, H0, f, lo, up)
        assert BH.same(got, ref), (lo is None, up is None)
        assert (ref["status"] == OK).all()


@pytest.mark.parametrize("n", EDGE_SHAPES)
def test_infinite_nan_pinned_and_crossed_bounds(qpb, n):
    B = EDGE_B
    H0, f, lb, ub = BH.family(B, n)
    lb, ub = lb.copy(), ub.copy()
    j = np.arange(B) % n
    q = np.arange(B)
    ub[q[0::5], j[0::5]] = np.inf
    lb[q[1::5], j[1::5]] = -np.inf
    ub[q[2::5], j[2::5]] = np.nan
    lb[q[3::5], j[3::5]] = np.nan
    pin = q[4::5]
    ub[pin, j[pin]] = lb[pin, j[pin]]  # pinned: lb = ub
    got, ref = _both(qpb, H0, f, lb, ub)
    assert BH.same(got, ref)
    # crossed bounds on every third QP: lb > ub on one variable
    lb2, ub2 = BH.family(B, n)[2].copy(), BH.family(B, n)[3].copy()
    lb2[::3, 0], ub2[::3, 0] = ub2[::3, 0] + 1.0, lb2[::3, 0] - 1.0
    got, ref = _both(qpb, H0, f, lb2, ub2)
    assert BH.same(got, ref)
    assert (ref["status"][::3] != OK).all() and (np.delete(ref["status"], np.s_[::3]) == OK).all()


@pytest.mark.parametrize("n", EDGE_SHAPES)
@pytest.mark.parametrize("max_iter", [1, 3])
def test_capped_iterations(qpb, n, max_iter):
    H0, f, lb, ub = BH.family(EDGE_B, n)
    got, ref = _both(qpb, H0, f, lb, ub, max_iter=max_iter)
    assert BH.same(got, ref)
    assert (ref["iters"] <= max_iter).all()


@pytest.mark.parametrize("n", EDGE_SHAPES)
def test_nan_in_one_f_leaves_the_other_qps_alone(qpb, n):
    B = EDGE_B
    H0, f, lb, ub = BH.family(B, n)
    f = f.copy()
    bad = 9
    f[bad, n // 2] = np.nan
    got, ref = _both(qpb, H0, f, lb, ub)
    assert BH.same(got, ref)
    assert got["status"][bad] != OK
    clean = _reference(qpb, B, n)
    per = {"x": n, "lam": 2 * n, "active": (2 * n + 31) // 32, "status": 1, "iters": 1}
    for k, w in per.items():
        a, c = got[k].reshape(B, w), clean[k].reshape(B, w)
        keep = np.arange(B) != bad
        assert BH.bits(np.ascontiguousarray(a[keep]), np.ascontiguousarray(c[keep])), k


@pytest.mark.parametrize("n", EDGE_SHAPES)
def test_non_spd_and_nan_h0(qpb, n):
    B = EDGE_B
    H0, f, lb, ub = BH.family(B, n)
    Hn = H0.copy()
    Hn[n - 1, n - 1] = -1.0  # indefinite
    got, ref = _both(qpb, Hn, f, lb, ub)
    assert BH.same(got, ref)
    assert (ref["status"] == NOT_SPD).all()
    Hn = H0.copy()
    Hn[n // 2, n // 2] = np.nan
    got, ref = _both(qpb, Hn, f, lb, ub)
    assert BH.same(got, ref)
    assert (ref["status"] != OK).all()


@pytest.mark.parametrize("n", [5, 16, 20, 33])
def test_a_qp_does_not_depend_on_its_batch(qpb, n):
    B = SC.batches(qpb)[-1]
    H0, f, lb, ub = BH.family(B, n)
    full = BH.solve(qpb, H0, f, lb, ub)
    per = {"x": n, "lam": 2 * n, "active": (2 * n + 31) // 32, "status": 1, "iters": 1}
    for k in (0, 130, B - 1):
        one = BH.solve(qpb, H0, f[k:k + 1], lb[k:k + 1], ub[k:k + 1])
        for name, w in per.items():
            assert BH.bits(one[name], np.ascontiguousarray(full[name].reshape(B, w)[k])), (k, name)


@pytest.mark.parametrize("n", [16, 20, 33])
def test_side_stream_and_host_call_give_the_same_bits(qpb, n):
    B = EDGE_B
    H0, f, lb, ub = BH.family(B, n)
    ref = _reference(qpb, B, n)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert BH.same(BH.solve(qpb, H0, f, lb, ub, stream=side), ref)
    qpb.release_stream_workspace(side)
    assert BH.same(BH.solve(qpb, H0, f, lb, ub, host=True), ref)
    assert BH.same(BH.solve(qpb, H0, f, None, ub, host=True), BH.solve(qpb, H0, f, None, ub))


def test_python_calls(qpb):
    n, B = 16, 5
    H0, f, lb, ub = BH.family(B, n)
    ref = _reference(qpb, B, n)
    sol = qpb.solve_box_shared(BH.dev(H0), BH.dev(f), BH.dev(lb), BH.dev(ub))
    torch.cuda.synchronize()
    assert sol.x.shape == (B, n) and sol.lam.shape == (B, 2 * n)
    assert np.array_equal(sol.x.cpu().numpy().ravel(), ref["x"])
    assert np.array_equal(sol.status.cpu().numpy(), ref["status"])
    hs = qpb.solve_box_shared_host(H0, f, lb, ub)
    assert np.array_equal(hs.x.ravel(), ref["x"]) and np.array_equal(hs.lam.ravel(), ref["lam"])
    with pytest.raises(ValueError):
        qpb.solve_box_shared(BH.dev(SC.expand(H0, B)), BH.dev(f))
