"""qpb.diff.solve_box with a 2-D H -- one matrix for the whole batch -- against
the same call on an expanded, contiguous (B, n, n) leaf: x, f.grad, lb.grad and
ub.grad are bitwise equal; H.grad is (n, n), symmetric bit for bit, and agrees
with the batched H.grad added over the batch with math.fsum within the derived
bound of tests/shared_cases.py (sum_bound).  A bound passed as None gets no
gradient, no backward call is made when nothing requires grad, and -- the point
of the feature -- at n = 32, B = 2 048 the 2-D forward and backward never
allocate a (B, n, n) tensor: torch's peak over the two passes, from after the
inputs exist, stays below B n n 8 bytes = 16.8 MB.
"""
import numpy as np
import pytest

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


@pytest.mark.parametrize("n", [5, 16, 20])
def test_two_d_h_against_expanded(qpb, n):
    B = SC.batches(qpb)[-1]
    H0, f, lb, ub = BH.family(B, n)
    w = _dev(np.random.default_rng([BH.SEED, n]).standard_normal((B, n)))
    H2, f2, l2, u2 = (_dev(a).requires_grad_(True) for a in (H0, f, lb, ub))
    x2, st2 = qpb.diff.solve_box(H2, f2, l2, u2)
    (w * x2).sum().backward()
    H3, f3, l3, u3 = (_dev(a).requires_grad_(True) for a in (SC.expand(H0, B), f, lb, ub))
    x3, st3 = qpb.diff.solve_box(H3, f3, l3, u3)
    (w * x3).sum().backward()
    torch.cuda.synchronize()
    assert (st2.cpu().numpy() == 0).all() and not st2.requires_grad
    assert H2.grad.shape == (n, n) and H3.grad.shape == (B, n, n)
    assert _eq(x2, x3) and _eq(st2, st3)
    assert _eq(f2.grad, f3.grad) and _eq(l2.grad, l3.grad) and _eq(u2.grad, u3.grad)
    assert bool((l2.grad != 0).any()) and bool((u2.grad != 0).any())  # both bounds' gradients take part
    none = np.zeros((B, 0))
    bound = SC.sum_bound(x2.detach().cpu().numpy(), f2.grad.cpu().numpy(), none, none, np.zeros((B, 0), bool),
                         np.ones(B, bool))[0]
    g = H2.grad.cpu().numpy()
    delta = np.abs(g - SC.fsum0(H3.grad.cpu().numpy()))
    with np.errstate(invalid="ignore", divide="ignore"):
        print(f"n={n}: worst |delta| / bound of H.grad {np.nanmax(np.where(bound > 0, delta / bound, 0)):.3g}")
    assert (delta <= bound).all()
    assert np.array_equal(g.view(np.uint8), np.ascontiguousarray(g.T).view(np.uint8))


@pytest.mark.parametrize("absent", ["lb", "ub"])
def test_a_bound_passed_as_none_gets_no_gradient(qpb, absent):
    n, B = 16, 67
    H0, f, lb, ub = BH.family(B, n)
    H2, f2 = _dev(H0).requires_grad_(True), _dev(f).requires_grad_(True)
    kept = _dev(ub if absent == "lb" else lb).requires_grad_(True)
    args = (None, kept) if absent == "lb" else (kept, None)
    x, st = qpb.diff.solve_box(H2, f2, *args)
    x.sum().backward()
    H3, f3 = _dev(SC.expand(H0, B)).requires_grad_(True), _dev(f).requires_grad_(True)
    kept3 = _dev(ub if absent == "lb" else lb).requires_grad_(True)
    x3, _ = qpb.diff.solve_box(H3, f3, *((None, kept3) if absent == "lb" else (kept3, None)))
    x3.sum().backward()
    torch.cuda.synchronize()
    assert (st == qpb.OK).all() and _eq(x, x3)
    assert H2.grad.shape == (n, n) and _eq(f2.grad, f3.grad) and _eq(kept.grad, kept3.grad)
    assert bool((kept.grad != 0).any())


def test_no_backward_call_without_a_gradient(qpb, monkeypatch):
    n, B = 16, 5
    H0, f, lb, ub = BH.family(B, n)
    calls = []
    real = qpb.solve_box_shared_backward
    monkeypatch.setattr(qpb, "solve_box_shared_backward", lambda *a, **k: calls.append(k.get("need")) or real(*a, **k))
    x, st = qpb.diff.solve_box(_dev(H0), _dev(f), _dev(lb), _dev(ub))
    assert not x.requires_grad and calls == []
    # a gradient that no input takes: backward returns before the call
    x, st = qpb.diff.solve_box(_dev(H0), _dev(f), None, None)
    assert not x.requires_grad and calls == []
    # only what is wanted is asked for
    ft = _dev(f).requires_grad_(True)
    x, st = qpb.diff.solve_box(_dev(H0), ft, _dev(lb), _dev(ub))
    x.sum().backward()
    torch.cuda.synchronize()
    assert calls == [["f"]] and ft.grad is not None


def test_no_per_qp_matrix_is_allocated(qpb):
    B, n = 2048, 32
    H0 = BH.family(67, n)[0]
    rs = np.random.default_rng(BH.SEED)
    f = _dev(rs.uniform(-1e2, 1e2, size=(B, n))).requires_grad_(True)
    lb = _dev(-rs.uniform(0.5, 1.5, size=(B, n))).requires_grad_(True)
    ub = _dev(rs.uniform(0.5, 1.5, size=(B, n))).requires_grad_(True)
    H = _dev(H0).requires_grad_(True)
    w = torch.ones((B, n), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()  # the inputs exist
    x, st = qpb.diff.solve_box(H, f, lb, ub)
    (w * x).sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"peak over the 2-D forward and backward: {peak / 1e6:.2f} MB new "
          f"(a (B, n, n) tensor: {B * n * n * 8 / 1e6:.1f} MB)")
    assert peak < B * n * n * 8
    assert H.grad.shape == (n, n) and f.grad.shape == (B, n) and lb.grad.shape == (B, n)
    assert (st == 0).all() and torch.isfinite(H.grad).all()
