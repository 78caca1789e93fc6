"""qpb_factor_shared_backward and qpb_solve_factored_backward on the GPU.

The reference throughout is qpb_solve_shared_backward with both operands shared
(shared_cases.shared_backward(qpb, 3, H0, A0, ...)) on the same x, lam, active,
status and cotangent, and the comparison is bit for bit: the factored forms run
the unfactored kernels' operations on the unfactored kernels' numbers, so the
numerical bars of tests/test_gpu_backward*.py are inherited, not re-argued.
"""
import ctypes
import itertools

import numpy as np
import pytest

import bwd_cases as BC
import factored_bwd_cases as FB
import shared_cases as SC
from bwd_harness import NAMES, dev as _dev

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

OK, NOT_SPD = 0, 2
SHARED_BOTH = SC.SHARED_H | SC.SHARED_A


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    assert q.NOT_SPD == NOT_SPD and q.OK == OK
    return q


_CASES = {}


def _case(qpb, B, n, m, meq):
    """One case's inputs, its forward on the GPU (qpb_solve_shared), a seeded
    cotangent, the buffer and the reference backward: once, shared, never modified."""
    key = (B, n, m, meq)
    if key not in _CASES:
        H0, f, A0, b = SC.family(B, n, m, meq)
        sol = qpb.solve_shared(_dev(H0), _dev(f), _dev(A0) if m else None, _dev(b) if m else None, meq)
        torch.cuda.synchronize()
        x, lam, act, st = (t.cpu().numpy() for t in (sol.x, sol.lam, sol.active, sol.status))
        assert (st == OK).all(), st
        g = np.random.default_rng([SC.SEED, B, n, m, meq, 16]).standard_normal((B, n))
        ref = SC.shared_backward(qpb, SHARED_BOTH, H0, A0, x, lam, act, st, g)
        F = FB.factor(qpb, H0, A0)
        assert F.result()[1] == OK
        mask = qpb.active_mask_to_bool(act, m) if m else np.zeros((B, 0), bool)
        _CASES[key] = dict(H0=H0, A0=A0, x=x, lam=lam, act=act, st=st, g=g, ref=ref, F=F, mask=mask)
    return _CASES[key]


def _run(qpb, c, **kw):
    x, lam, act = kw.pop("x", c["x"]), kw.pop("lam", c["lam"]), kw.pop("act", c["act"])
    st = kw.pop("st", c["st"])
    return FB.factored_backward(qpb, c["F"], x, lam, act, st, c["g"], **kw)


@pytest.mark.parametrize("n,m,meq", SC.SHAPES)
def test_after_a_forward_solve(qpb, n, m, meq):
    for B in SC.batches(qpb):
        c = _case(qpb, B, n, m, meq)
        got = _run(qpb, c)
        FB.same(got, c["ref"], (B, n, m))
        assert FB.bits(got["H"], np.ascontiguousarray(got["H"].T)), (B, "gH is not symmetric bit for bit")
    # the Python call, at the last batch
    sol = qpb.Solution(_dev(c["x"]), _dev(c["lam"]) if m else None, _dev(c["act"]) if m else None, _dev(c["st"]), None)
    F = qpb.factor_shared_backward(_dev(c["H0"]), _dev(c["A0"]) if m else None)
    assert isinstance(F, qpb.BackwardFactor) and (F.n, F.m) == (n, m)
    out = qpb.solve_factored_backward(F, sol, _dev(c["g"]))
    torch.cuda.synchronize()
    assert int(F.status.cpu()[0]) == OK
    assert FB.bits(F.fac.cpu().numpy(), c["F"].result()[0])
    for k, t in zip(NAMES, out):
        if k in c["ref"]:
            assert FB.bits(t.cpu().numpy(), c["ref"][k]), ("python", k)
        else:
            assert t is None, k


def _hand_made(qpb, c, k0, where):
    """The shared H and A are QP k0's of a hand-made case; every QP of the case
    supplies its own mask, x, lam and g (the backward is a function of the
    caller's mask: any of them is a legal input)."""
    H0, A0 = np.ascontiguousarray(c.H[k0]), np.ascontiguousarray(c.A[k0])
    act = BC.words(c.mask)
    ref = SC.shared_backward(qpb, SHARED_BOTH, H0, A0, c.x, c.lam, act, None, c.g)
    F = FB.factor(qpb, H0, A0)
    assert F.result()[1] == OK, where
    got = FB.factored_backward(qpb, F, c.x, c.lam, act, None, c.g)
    FB.same(got, ref, where)


@pytest.mark.parametrize("n,m", BC.ALL_ROUTES)
def test_every_form_sizes(qpb, n, m):
    _hand_made(qpb, BC.sizes(n, m), 0, ("sizes", n, m))


@pytest.mark.parametrize("n,m", BC.FORM_ROUTES)
def test_every_form_overfull(qpb, n, m):
    _hand_made(qpb, BC.overfull(n, m), 0, ("overfull", n, m))


@pytest.mark.parametrize("n,m", BC.COND_SHAPES)
def test_every_form_conditioned(qpb, n, m):
    """QP 0's H has cond 1e3; the last QP's has cond(H) = 1e10 with |W| = n: both as the shared pair."""
    c = BC.conditioned(n, m)
    _hand_made(qpb, c, 0, ("conditioned", n, m, 0))
    _hand_made(qpb, c, len(c.H) - 1, ("conditioned", n, m, "cond 1e10"))


@pytest.mark.parametrize("n,m,meq", [(5, 9, 2), (16, 32, 4), (20, 40, 4)])
def test_every_need_subset(qpb, n, m, meq):
    B = SC.batches(qpb)[-1]
    c = _case(qpb, B, n, m, meq)
    full = _run(qpb, c)
    FB.same(full, c["ref"], "full")
    for r in range(1, 4):
        for need in itertools.combinations(NAMES, r):
            got = _run(qpb, c, need=need)
            assert set(got) == set(need)
            for k in need:
                assert FB.bits(got[k], full[k]), (need, k)


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
    ref = SC.shared_backward(qpb, SHARED_BOTH, c["H0"], c["A0"], x, lam, c["act"], st, c["g"])
    got = _run(qpb, c, x=x, lam=lam, st=st)
    FB.same(got, ref, "poison")
    for k in got:
        assert np.isfinite(got[k]).all(), k
    assert not got["f"][bad].any() and not got["b"][bad].any()


@pytest.mark.parametrize("n,m,meq", [(16, 32, 4), (20, 40, 4)])
def test_status_null(qpb, n, m, meq):
    c = _case(qpb, 67, n, m, meq)
    FB.same(_run(qpb, c, st=None), _run(qpb, c), "status NULL")


@pytest.mark.parametrize("n,m,meq", [(16, 32, 4), (32, 64, 8)])
def test_reproducible(qpb, n, m, meq):
    B = SC.batches(qpb)[-1]
    c = _case(qpb, B, n, m, meq)
    before = c["F"].result()[0]
    first = _run(qpb, c)
    again = _run(qpb, c)
    qpb.release_workspaces()
    fresh = _run(qpb, c)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    other = _run(qpb, c, stream=side)
    qpb.release_stream_workspace(side)
    for name, got in (("again", again), ("after release_workspaces", fresh), ("side stream", other)):
        FB.same(got, first, name)
    # the buffer is only read, and a second factor call writes the same bytes
    assert FB.bits(c["F"].result()[0], before)
    assert FB.bits(FB.factor(qpb, c["H0"], c["A0"]).result()[0], before)
    # factor and solve queued on a side stream with no host synchronisation between them
    F2 = FB.factor(qpb, c["H0"], c["A0"], stream=side)
    queued = FB.factored_backward(qpb, F2, c["x"], c["lam"], c["act"], c["st"], c["g"], stream=side)
    FB.same(queued, first, "queued behind the factor call")
    assert FB.bits(F2.result()[0], before)


@pytest.mark.parametrize("n,m,meq", [(5, 9, 2), (20, 40, 4)])
def test_not_spd(qpb, n, m, meq):
    c = _case(qpb, 5, n, m, meq)
    nan_h = c["H0"].copy()
    nan_h[n // 2, n // 2] = np.nan
    for H in (-np.eye(n), nan_h):
        F = FB.factor(qpb, H, c["A0"])
        assert F.result()[1] == NOT_SPD
        for st in (None, c["st"]):
            got = FB.factored_backward(qpb, F, c["x"], c["lam"], c["act"], st, c["g"])
            assert set(got) == set(NAMES)
            for k in got:
                assert (got[k] == 0).all(), (k, "status NULL" if st is None else "status OK")
    F = FB.factor(qpb, c["H0"], c["A0"], fstatus=False)  # fstatus NULL
    torch.cuda.synchronize()
    assert FB.bits(F.fac.cpu().numpy(), c["F"].result()[0])


def test_limits(qpb):
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")  # noqa: E731
    eye = lambda n: torch.eye(n, dtype=torch.float64, device="cuda")  # noqa: E731
    for H, A in ((eye(33), None), (eye(16), z(65, 16))):
        with pytest.raises(qpb.QPBError) as e:
            qpb.factor_shared_backward(H, A)
        assert e.value.code == qpb.ERR_UNSUPPORTED
    for n, m in ((33, 0), (16, 65)):
        d = qpb.Desc(n, m, 4, 0, 0, 0.0)
        p = ctypes.c_void_p(z(16).data_ptr())
        rc = qpb.lib().qpb_solve_factored_backward(ctypes.byref(d), *([p] * 10), None)
        assert rc == qpb.ERR_UNSUPPORTED, (n, m)
    # a buffer of another length is refused by the Python call
    c = _case(qpb, 5, 5, 9, 2)
    sol = qpb.Solution(_dev(c["x"]), _dev(c["lam"]), _dev(c["act"]), None, None)
    good = qpb.factor_shared_backward(_dev(c["H0"]), _dev(c["A0"]))
    with pytest.raises(ValueError):
        qpb.solve_factored_backward(qpb.BackwardFactor(good.fac[:-2], 5, 9, good.status), sol, _dev(c["g"]))
    forward = qpb.factor_shared(_dev(c["H0"]), _dev(c["A0"]))
    if forward.fac.numel() != good.fac.numel():
        with pytest.raises(ValueError):
            qpb.solve_factored_backward(qpb.BackwardFactor(forward.fac, 5, 9, forward.status), sol, _dev(c["g"]))
    # a misaligned bfac, in both calls
    buf = z(qpb.factor_backward_doubles(5, 9) + 2)
    off = ctypes.c_void_p(buf.data_ptr() + 8)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = qpb.lib().qpb_factor_shared_backward(5, 9, ptr(_dev(c["H0"])), ptr(_dev(c["A0"])), off, None, None)
    assert rc == qpb.ERR_INVALID_ARG and b"16-byte" in qpb.lib().qpb_last_error()
    d = qpb.Desc(5, 9, 5, 0, 0, 0.0)
    gf = z(5, 5)
    rc = qpb.lib().qpb_solve_factored_backward(ctypes.byref(d), off, ptr(sol.x), ptr(sol.lam), ptr(sol.active), None,
                                               ptr(_dev(c["g"])), None, ptr(gf), None, None, None)
    assert rc == qpb.ERR_INVALID_ARG and b"16-byte" in qpb.lib().qpb_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", [3, 20])
def test_without_rows(qpb, n):
    """m == 0: gA and gb are ignored, gH and gf are the reference's."""
    B = 67
    c = _case(qpb, B, n, 0, 0)
    assert set(c["ref"]) == {"H", "f"}
    FB.same(_run(qpb, c), c["ref"], ("m == 0", n))
    # gA and gb given all the same: not written
    d = qpb.Desc(n, 0, B, 0, 0, 0.0)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    gH, gf = torch.empty(n, n, dtype=torch.float64, device="cuda"), torch.empty(B, n, dtype=torch.float64, device="cuda")
    junk = torch.full((64,), 7.0, dtype=torch.float64, device="cuda")
    x, g = _dev(c["x"]), _dev(c["g"])
    rc = qpb.lib().qpb_solve_factored_backward(ctypes.byref(d), ptr(c["F"].fac), ptr(x), None, None, None, ptr(g),
                                               ptr(gH), ptr(gf), ptr(junk), ptr(junk), None)
    assert rc == 0, qpb.lib().qpb_last_error()
    torch.cuda.synchronize()
    assert (junk == 7.0).all()
    assert FB.bits(gH.cpu().numpy(), c["ref"]["H"]) and FB.bits(gf.cpu().numpy(), c["ref"]["f"])
