"""qpb_solve_box_shared_backward on the GPU: the gradients of a box solve whose H
is one matrix for the whole batch.

Reference: qpb_solve_box_backward on shared_cases.expand(H0, B), fed the same
x, active, status and (seeded normal) cotangent.
  gf, glb, gub    bitwise equal.
  gH (n, n)       against the reference's per-QP gH added on the host with
                  math.fsum (shared_cases.fsum0): elementwise |delta| <=
                  shared_cases.sum_bound(x, gf, no gb, no lam, no mask, ok)[0] =
                  (B + 4) 2^-53 sum_k 1/2 (|dx_i x_j| + |x_i dx_j|), the derived
                  bound of the same sum kernel in qpb_solve_shared_backward (the
                  worst case of any order of B additions plus one rounding per
                  product; derived, not measured).  The worst ratio is printed.
  symmetry        gH == gH.T bitwise.
  need            every subset: gf NULL goes through the workspace, gH NULL is
                  pass 1 alone.
  reproducible    two runs, a run after release_workspaces() and a run on a
                  side stream give the same bits; so does the _host call.
  poison          QPs with status 1 and NaN in x contribute exactly 0.
  hand-made masks no bit, all bits, both bits of a variable, bits >= 2n.
Worst observed |delta| / bound on an MI355X: 0.22 (n = 32; 0.0012 at n = 1, 0.14 to 0.22 over the
other shapes), 4.3e-3 with poisoned QPs, 0.051 on the hand-made masks, 1.3e-6 at 65 536 QPs
(tools/ab_box_shared.py): the matrix cores accumulate each product unrounded.
"""
import itertools

import numpy as np
import pytest

import box_shared_harness as BH
import shared_cases as SC
from box_bwd_oracle import NAMES

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

OK = 0
SHAPES = BH.DENSE_N + BH.WAVE_N


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    return q


_CASES = {}


def _case(qpb, B, n):
    """One case's inputs, its forward on the GPU (qpb_solve_box_shared), the
    cotangent and the reference backward on copies: once, shared, never modified."""
    if (B, n) not in _CASES:
        H0, f, lb, ub = BH.family(B, n)
        fwd = BH.solve(qpb, H0, f, lb, ub)
        x, act, st = fwd["x"].reshape(B, n), fwd["active"].reshape(B, -1), fwd["status"]
        assert (st == OK).all(), st
        g = np.random.default_rng([BH.SEED, B, n]).standard_normal((B, n))
        ref = BH.backward(qpb, SC.expand(H0, B), x, act, st, g)
        _CASES[(B, n)] = dict(H0=H0, x=x, act=act, st=st, g=g, ref=ref)
    return _CASES[(B, n)]


def _bound(x, gf, ok):
    B = x.shape[0]
    none = np.zeros((B, 0))
    return SC.sum_bound(x, gf, none, none, np.zeros((B, 0), bool), ok)[0]


def _check(got, ref, bound, where):
    """got (shared) against the per-QP reference; returns the worst |delta| / bound of gH."""
    worst = 0.0
    for k in got:
        if k != "H":
            assert BH.bits(got[k], ref[k]), (where, k, "per-QP output differs")
            continue
        want = SC.fsum0(ref["H"])
        delta = np.abs(got["H"] - want)
        assert np.isfinite(got["H"]).all(), where
        assert (delta <= bound).all(), (where, float((delta - bound).max()))
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(bound > 0, delta / bound, 0.0)
        worst = float(r.max())
        assert BH.bits(got["H"], np.ascontiguousarray(got["H"].T)), (where, "gH is not symmetric bit for bit")
    return worst


@pytest.mark.parametrize("n", SHAPES)
def test_outputs_against_box_backward_on_copies(qpb, n):
    worst = 0.0
    for B in SC.batches(qpb):
        c = _case(qpb, B, n)
        got = BH.backward(qpb, c["H0"], c["x"], c["act"], c["st"], c["g"])
        assert set(got) == set(NAMES) and got["H"].shape == (n, n)
        worst = max(worst, _check(got, c["ref"], _bound(c["x"], c["ref"]["f"], np.ones(B, bool)), B))
    print(f"n={n}: worst |delta| / bound of the summed gH {worst:.3g}")


@pytest.mark.parametrize("n", [5, 16, 20])
def test_every_need_subset(qpb, n):
    B = SC.batches(qpb)[-1]
    c = _case(qpb, B, n)
    full = BH.backward(qpb, c["H0"], c["x"], c["act"], c["st"], c["g"])
    for r in range(1, 4):
        for need in itertools.combinations(NAMES, r):
            got = BH.backward(qpb, c["H0"], c["x"], c["act"], c["st"], c["g"], need=need)
            assert set(got) == set(need)
            for k in need:
                assert BH.bits(got[k], full[k]), (need, k)


@pytest.mark.parametrize("n", [16, 32])
def test_reproducible(qpb, n):
    B = SC.batches(qpb)[-1]
    c = _case(qpb, B, n)
    run = lambda **kw: BH.backward(qpb, c["H0"], c["x"], c["act"], c["st"], c["g"], **kw)  # noqa: E731
    first, again = run(), run()
    qpb.release_workspaces()
    fresh = run()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    other = run(stream=side)
    qpb.release_stream_workspace(side)
    host = run(host=True)
    only_h = run(need=("H",), host=True)
    for name, got in (("again", again), ("after release_workspaces", fresh), ("side stream", other), ("host", host),
                      ("host, gH alone", only_h)):
        for k in got:
            assert BH.bits(got[k], first[k]), (name, k)


@pytest.mark.parametrize("n", [5, 16, 20])
def test_status_none(qpb, n):
    B = 67
    c = _case(qpb, B, n)
    with_st = BH.backward(qpb, c["H0"], c["x"], c["act"], c["st"], c["g"])
    without = BH.backward(qpb, c["H0"], c["x"], c["act"], None, c["g"])
    assert BH.same(with_st, without)


@pytest.mark.parametrize("n", [5, 16, 20])
def test_poisoned_qps_contribute_nothing(qpb, n):
    B = SC.batches(qpb)[-1]
    c = _case(qpb, B, n)
    bad = np.zeros(B, bool)
    bad[::7] = True
    x, st = c["x"].copy(), c["st"].copy()
    st[bad] = 1
    x[bad] = np.nan
    got = BH.backward(qpb, c["H0"], x, c["act"], st, c["g"])
    ref = c["ref"]
    keep = {k: np.where(bad.reshape((B,) + (1,) * (ref[k].ndim - 1)), 0.0, ref[k]) for k in ref}
    worst = _check(got, keep, _bound(c["x"], ref["f"], ~bad), "poison")
    print(f"n={n} poisoned: worst |delta| / bound {worst:.3g}")
    # all poisoned: exactly 0
    st[:] = 1
    x[:] = np.nan
    got = BH.backward(qpb, c["H0"], x, c["act"], st, c["g"])
    assert all((v == 0.0).all() and not np.signbit(v).any() for v in got.values())


@pytest.mark.parametrize("n", [5, 16, 20])
def test_hand_made_masks(qpb, n):
    B = 67
    c = _case(qpb, B, n)
    w = (2 * n + 31) // 32
    act = np.zeros((B, w), dtype=np.uint32)
    full = (1 << (2 * n)) - 1
    words = lambda v: [(v >> (32 * i)) & 0xFFFFFFFF for i in range(w)]  # noqa: E731
    for q in range(B):
        j = q % n
        kind = q % 4
        v = 0 if kind == 0 else full if kind == 1 else (1 << j) | (1 << (n + j)) if kind == 2 else (1 << ((q * 5) % n))
        if kind == 3 and 2 * n < 32 * w:
            v |= ((1 << (32 * w)) - 1) & ~full  # bits >= 2n of the last word: ignored
        act[q] = words(v)
    act = act.view(np.int32)
    ref = BH.backward(qpb, SC.expand(c["H0"], B), c["x"], act, c["st"], c["g"])
    got = BH.backward(qpb, c["H0"], c["x"], act, c["st"], c["g"])
    worst = _check(got, ref, _bound(c["x"], ref["f"], np.ones(B, bool)), "masks")
    assert (ref["f"][1::4] == 0.0).all() and (ref["lb"][0::4] == 0.0).all()  # all fixed: dx = 0; none fixed: no bound
    print(f"n={n} hand-made masks: worst |delta| / bound {worst:.3g}")


def test_python_call_and_limit(qpb):
    n, B = 16, 67
    c = _case(qpb, B, n)
    sol = qpb.Solution(BH.dev(c["x"]), None, BH.dev(c["act"]), BH.dev(c["st"]), None)
    first = BH.backward(qpb, c["H0"], c["x"], c["act"], c["st"], c["g"])
    gH, gf, glb, gub = qpb.solve_box_shared_backward(BH.dev(c["H0"]), sol, BH.dev(c["g"]))
    torch.cuda.synchronize()
    assert gH.shape == (n, n) and gf.shape == glb.shape == gub.shape == (B, n)
    for k, t in zip(NAMES, (gH, gf, glb, gub)):
        assert BH.bits(t.cpu().numpy(), first[k]), k
    got = qpb.solve_box_shared_backward(BH.dev(c["H0"]), sol, BH.dev(c["g"]), need=("lb",))
    assert [t is None for t in got] == [True, True, False, True]
    hs = qpb.solve_box_shared_backward_host(c["H0"], qpb.Solution(c["x"], None, c["act"], c["st"], None), c["g"])
    for k, t in zip(NAMES, hs):
        assert BH.bits(t, first[k]), k
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")  # noqa: E731
    sol33 = qpb.Solution(z(4, 33), None, torch.zeros((4, 3), dtype=torch.int32, device="cuda"), None, None)
    with pytest.raises(qpb.QPBError) as e:
        qpb.solve_box_shared_backward(torch.eye(33, dtype=torch.float64, device="cuda"), sol33, z(4, 33))
    assert e.value.code == qpb.ERR_UNSUPPORTED
