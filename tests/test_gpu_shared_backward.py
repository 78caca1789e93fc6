"""qpb_solve_shared_backward on the GPU: the gradients of a solve whose H
and / or A is one matrix for the whole batch.

Reference: qpb_solve_backward on materialised copies of the shared operands
(tests/bwd_harness.py), fed the same x, lam, active, status and cotangent.
  per-QP outputs  gf, gb and the gradient of a batched operand: bitwise equal.
  summed outputs  the gradient of a shared operand, against the reference's
                  per-QP outputs added on the host with math.fsum: elementwise
                  |delta| <= (B + 4) 2^-53 T, T the sum over k of the absolute
                  values of the two products of each term, from x, gf, gb and
                  lam on the host (shared_cases.sum_bound: the worst case of any
                  order of B additions plus one rounding per product; derived,
                  not measured).  The worst observed ratio is printed.
  symmetry        gH == gH.T bitwise.
  reproducible    two runs, a run after release_workspaces() and a run on a
                  side stream give the same bits.
  poison          QPs with status 1 and NaN in x and lam, others with 1e300 in
                  lam outside W: the sums stay finite and equal the sums over
                  the remaining QPs.
Worst observed |delta| / bound on an MI355X: 0.38 (n = 32, m = 64, at B = 1, where
the bound is five roundings; 0.04 to 0.38 over the shapes), 5.3e-3 with poisoned
QPs at B = 293, 3.5e-6 at 65 536 QPs (tools/ab_shared.py): the matrix cores
accumulate each product unrounded.
"""
import itertools

import numpy as np
import pytest

import shared_cases as SC
from bwd_harness import NAMES
from bwd_harness import backward as _backward, dev as _dev

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

OK = 0


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    return q


_CASES = {}


def _case(qpb, B, n, m, meq):
    """One case's inputs, its forward on the GPU (qpb_solve_shared), the
    cotangent and the reference backward on copies: once, shared, never modified."""
    key = (B, n, m, meq)
    if key not in _CASES:
        H0, f, A0, b = SC.family(B, n, m, meq)
        sol = qpb.solve_shared(_dev(H0), _dev(f), _dev(A0) if m else None, _dev(b) if m else None, meq)
        torch.cuda.synchronize()
        x, lam, act, st = (t.cpu().numpy() for t in (sol.x, sol.lam, sol.active, sol.status))
        assert (st == OK).all(), st
        g = np.random.default_rng([SC.SEED, B, n, m, meq]).standard_normal((B, n))
        ref = _backward(qpb, SC.expand(H0, B), SC.expand(A0, B), x, lam, act, st, g)
        mask = qpb.active_mask_to_bool(act, m) if m else np.zeros((B, 0), bool)
        _CASES[key] = dict(H0=H0, A0=A0, x=x, lam=lam, act=act, st=st, g=g, ref=ref, mask=mask)
    return _CASES[key]


def _run(qpb, c, shared, B, **kw):
    x, lam, act = kw.pop("x", c["x"]), kw.pop("lam", c["lam"]), kw.pop("act", c["act"])
    st = kw.pop("st", c["st"])
    return SC.shared_backward(qpb, shared, SC.operand(c["H0"], B, shared & 1), SC.operand(c["A0"], B, shared & 2),
                              x, lam, act, st, c["g"], **kw)


def _bits(a, b):
    return np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _check(got, ref, shared, bounds, where, m):
    """got against the per-QP reference `ref` (all four arrays); returns the worst |delta| / bound."""
    worst = 0.0
    for k in got:
        summed = (k == "H" and shared & 1) or (k == "A" and shared & 2)
        if not summed:
            assert _bits(got[k], ref[k]), (where, k, "per-QP output differs")
            continue
        want = SC.fsum0(ref[k])
        bound = bounds[0] if k == "H" else bounds[1]
        delta = np.abs(got[k] - want)
        assert np.isfinite(got[k]).all(), (where, k)
        assert (delta <= bound).all(), (where, k, float((delta - bound).max()))
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(bound > 0, delta / bound, 0.0)
        worst = max(worst, float(r.max()) if r.size else 0.0)
        if k == "H":
            assert _bits(got[k], np.ascontiguousarray(got[k].T)), (where, "gH is not symmetric bit for bit")
    return worst


@pytest.mark.parametrize("n,m,meq", SC.SHAPES)
def test_outputs_against_backward_on_copies(qpb, n, m, meq):
    worst = 0.0
    for B in SC.batches(qpb):
        c = _case(qpb, B, n, m, meq)
        ref = c["ref"]
        bounds = SC.sum_bound(c["x"], ref["f"], ref.get("b", np.zeros((B, 0))), c["lam"], c["mask"],
                              np.ones(B, bool))
        for shared in (1, 2, 3):
            got = _run(qpb, c, shared, B)
            assert got.keys() == ref.keys()
            worst = max(worst, _check(got, ref, shared, bounds, (B, shared), m))
    print(f"n={n} m={m} meq={meq}: worst |delta| / bound of a summed gradient {worst:.3g}")


@pytest.mark.parametrize("n,m,meq", [(5, 9, 2), (16, 32, 4), (20, 40, 4)])
def test_every_need_subset_with_a_summed_output(qpb, n, m, meq):
    """gf and / or gb NULL: dx and dlam then go through the workspace."""
    B = SC.batches(qpb)[-1]
    c = _case(qpb, B, n, m, meq)
    full = {s: _run(qpb, c, s, B) for s in (1, 2, 3)}
    for r in range(1, 4):
        for need in itertools.combinations(NAMES, r):
            for shared in (1, 2, 3):
                if not (("H" in need and shared & 1) or ("A" in need and shared & 2)):
                    continue
                got = _run(qpb, c, shared, B, need=need)
                assert set(got) == set(need)
                for k in need:
                    assert _bits(got[k], full[shared][k]), (need, shared, k)


@pytest.mark.parametrize("n,m,meq", [(16, 32, 4), (32, 64, 8)])
def test_reproducible(qpb, n, m, meq):
    B = SC.batches(qpb)[-1]
    c = _case(qpb, B, n, m, meq)
    first = _run(qpb, c, 3, B)
    again = _run(qpb, c, 3, B)
    qpb.release_workspaces()
    fresh = _run(qpb, c, 3, B)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    other = _run(qpb, c, 3, B, stream=side)
    qpb.release_stream_workspace(side)
    for name, got in (("again", again), ("after release_workspaces", fresh), ("side stream", other)):
        for k in first:
            assert _bits(got[k], first[k]), (name, k)


@pytest.mark.parametrize("n,m,meq", [(5, 9, 2), (16, 32, 4), (20, 40, 4)])
def test_poisoned_qps_contribute_nothing(qpb, n, m, meq):
    B = SC.batches(qpb)[-1]
    c = _case(qpb, B, n, m, meq)
    bad = np.zeros(B, bool)
    bad[::7] = True
    x, lam, st = c["x"].copy(), c["lam"].copy(), c["st"].copy()
    st[bad] = 1
    x[bad] = np.nan
    lam[bad] = np.nan
    out_of_w = ~c["mask"] & ~bad[:, None]
    out_of_w[::2] = False
    assert out_of_w.any()
    lam[out_of_w] = 1e300
    got = _run(qpb, c, 3, B, x=x, lam=lam, st=st)
    ref = c["ref"]
    keep = {k: np.where(bad.reshape((B,) + (1,) * (ref[k].ndim - 1)), 0.0, ref[k]) for k in ref}
    bounds = SC.sum_bound(c["x"], ref["f"], ref["b"], c["lam"], c["mask"], ~bad)
    worst = _check(got, keep, 3, bounds, "poison", m)
    print(f"n={n} m={m} poisoned: worst |delta| / bound {worst:.3g}")


def test_status_none_and_python_call(qpb):
    n, m, meq, B = 16, 32, 4, 67
    c = _case(qpb, B, n, m, meq)
    with_st = _run(qpb, c, 3, B)
    without = _run(qpb, c, 3, B, st=None)
    for k in with_st:
        assert _bits(with_st[k], without[k]), k
    sol = qpb.Solution(_dev(c["x"]), _dev(c["lam"]), _dev(c["act"]), None, None)
    gH, gf, gA, gb = qpb.solve_shared_backward(_dev(c["H0"]), _dev(c["A0"]), sol, _dev(c["g"]))
    torch.cuda.synchronize()
    assert gH.shape == (n, n) and gA.shape == (m, n) and gf.shape == (B, n) and gb.shape == (B, m)
    for k, t in zip(NAMES, (gH, gf, gA, gb)):
        assert _bits(t.cpu().numpy(), with_st[k]), k
    # one operand batched: its gradient is per QP
    gH3, _, gA2, _ = qpb.solve_shared_backward(_dev(SC.expand(c["H0"], B)), _dev(c["A0"]), sol, _dev(c["g"]))
    torch.cuda.synchronize()
    assert gH3.shape == (B, n, n) and gA2.shape == (m, n)
    assert _bits(gH3.cpu().numpy(), c["ref"]["H"])


def test_unsupported_above_the_wave_classes(qpb):
    n, B = 33, 4
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")  # noqa: E731
    sol = qpb.Solution(z(B, n), None, None, None, None)
    with pytest.raises(qpb.QPBError) as e:
        qpb.solve_shared_backward(torch.eye(n, dtype=torch.float64, device="cuda"), None, sol, z(B, n))
    assert e.value.code == qpb.ERR_UNSUPPORTED and "shared" in str(e.value)
