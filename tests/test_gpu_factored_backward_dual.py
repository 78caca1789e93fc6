"""qpb_solve_factored_backward_dual on the GPU: the backward of a solve for a
loss that reads the multipliers too, on a buffer of qpb_factor_shared_backward --
the DU forms of the factored forms of both kernels of qpb_kkt_bwd.hip (n <= 16,
m <= 32: four QPs per wavefront, MR = 1 and 2, n == 16 and padded; the rest of
n <= 32, m <= 64: one QP per wavefront).

The reference throughout is qpb_solve_backward_dual with both operands shared
on the H and A the buffer was made from, for the same x, lam, active, status, gx
and glam, and the comparison is bit for bit on every output: the numerical bars
of tests/test_gpu_backward_dual.py are inherited, not re-argued.  One parity
run per kernel class is held against tests/dual_oracle.py as well, at the
project's X_TOL = 1e-6 and KKT_TOL = 1e-9 (tests/bwd_harness.py).

Every kind of input runs on all nine shapes, with two exceptions.  The oracle
parity run is one shape per kernel class.  The hand-made masks are
bwd_cases.sizes and bwd_cases.overfull on bwd_cases.ALL_ROUTES and FORM_ROUTES,
the smallest shapes that reach every MR / N16 / wave form, as in
tests/test_gpu_factored_backward.py: those cases are built for their own shapes
(integer rows, margins of the kept and skipped rows checked on the CPU).

Every call goes through the C-ABI into buffers of the test's own, filled with
0xA5 and fenced by guard words.  The batch of 67 leaves the four-per-wave kernel
a ragged last wave.
"""
import itertools

import numpy as np
import pytest

import bwd_cases as BC
import dual_oracle as DO
import dual_paths_harness as DP
import factored_bwd_cases as FB
import shared_cases as SC
from bwd_harness import KKT_TOL, NAMES, X_TOL, dev as _dev, rel as _rel

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

OK, MAX_ITER, NOT_SPD, NUMERICAL = 0, 1, 2, 4
B = 67
BOTH = SC.SHARED_H | SC.SHARED_A
# (n, m, meq): MR 1 padded, MR 1 / 2 at n = 16, meq = n | the wave kernel
DENSE_SHAPES = [(1, 2, 1), (5, 9, 2), (16, 16, 3), (16, 32, 4), (16, 32, 16)]
WAVE_SHAPES = [(16, 33, 0), (20, 40, 4), (32, 64, 8), (32, 64, 32)]
SHAPES = DENSE_SHAPES + WAVE_SHAPES
# the parity run against the numpy oracle, one shape per kernel class and load path: n < 16, n == 16 with two rows
# per lane, the wave kernel (every other test runs on all of SHAPES)
PATH_SHAPES = [(5, 9, 2), (16, 32, 4), (20, 40, 4)]


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    return q


_CASES = {}


def _case(qpb, n, m, meq):
    """One shape's shared H0 and A0, its forward on the GPU (qpb_solve_shared),
    seeded cotangents, the buffer and the reference: once, shared, never modified."""
    key = (n, m, meq)
    if key not in _CASES:
        H0, f, A0, b = SC.family(B, n, m, meq)
        sol = qpb.solve_shared(_dev(H0), _dev(f), _dev(A0), _dev(b), meq)
        torch.cuda.synchronize()
        x, lam, act, st = (t.cpu().numpy() for t in (sol.x, sol.lam, sol.active, sol.status))
        # (the comparisons are bit for bit whatever the status; the shapes that go to the oracle are all OK)
        assert (st == OK).all() if key in PATH_SHAPES else (st == OK).sum() > B // 2, st
        rng = np.random.default_rng([SC.SEED, B, n, m, meq, 20])
        g, gl = rng.standard_normal((B, n)), rng.standard_normal((B, m))
        ref = DP.dual(qpb, BOTH, H0, A0, x, lam, act, st, g, gl)
        F = FB.factor(qpb, H0, A0)
        assert F.result()[1] == OK
        _CASES[key] = dict(H0=H0, A0=A0, x=x, lam=lam, act=act, st=st, g=g, gl=gl, ref=ref, F=F,
                           mask=qpb.active_mask_to_bool(act, m))
    return _CASES[key]


def _run(qpb, c, **kw):
    x, lam, act = kw.pop("x", c["x"]), kw.pop("lam", c["lam"]), kw.pop("act", c["act"])
    st, gl = kw.pop("st", c["st"]), kw.pop("gl", c["gl"])
    return DP.factored_dual(qpb, c["F"], x, lam, act, st, c["g"], gl, **kw)


# ------------------------------------------------------- after a forward solve, every form
@pytest.mark.parametrize("n,m,meq", SHAPES)
def test_after_a_forward_solve(qpb, n, m, meq):
    c = _case(qpb, n, m, meq)
    got = _run(qpb, c)
    assert set(got) == set(NAMES)
    DP.same(got, c["ref"], (n, m, meq))
    assert DP.bits(got["H"], np.ascontiguousarray(got["H"].T)), "gH is not symmetric bit for bit"
    # the cotangent on lam is not a no-op, and without it the call is qpb_solve_factored_backward
    plain = FB.factored_backward(qpb, c["F"], c["x"], c["lam"], c["act"], c["st"], c["g"])
    DP.same(_run(qpb, c, gl=None), plain, "glam NULL")
    assert not DP.bits(got["f"], plain["f"])
    # the Python calls return the same bits
    sol = qpb.Solution(_dev(c["x"]), _dev(c["lam"]), _dev(c["act"]), _dev(c["st"]), None)
    F = qpb.factor_shared_backward(_dev(c["H0"]), _dev(c["A0"]))
    out = qpb.solve_factored_backward_dual(F, sol, _dev(c["g"]), _dev(c["gl"]))
    none = qpb.solve_factored_backward_dual(F, sol, _dev(c["g"]), None)
    torch.cuda.synchronize()
    DP.same({k: t.cpu().numpy() for k, t in zip(NAMES, out)}, c["ref"], "python")
    DP.same({k: t.cpu().numpy() for k, t in zip(NAMES, none)}, plain, "python, glam None")


# ------------------------------------------------------- parity with the numpy oracle, one per kernel class
@pytest.mark.parametrize("n,m,meq", PATH_SHAPES)
def test_parity_and_certificate(qpb, n, m, meq):
    c = _case(qpb, n, m, meq)
    out = _run(qpb, c)
    ref = [DO.backward(c["H0"], c["x"][i], c["lam"][i], c["A0"], c["mask"][i], c["g"][i], c["gl"][i]) for i in range(B)]
    ref = {k: np.array([r[j] for r in ref]) for j, k in enumerate(NAMES)}
    errs = {"f": float(_rel(out["f"], ref["f"]).max()), "b": float(_rel(out["b"], ref["b"]).max()),
            "H": float(_rel(out["H"][None], SC.fsum0(ref["H"])[None])[0]),
            "A": float(_rel(out["A"][None], SC.fsum0(ref["A"])[None])[0])}
    cert = np.array([DO.certificate(c["H0"], c["A0"], c["mask"][i], c["g"][i], c["gl"][i], out["f"][i], out["b"][i])
                     for i in range(B)])
    print(f"({n},{m},{meq}): active rows {c['mask'].sum(axis=1).min()}..{c['mask'].sum(axis=1).max()} errors {errs} "
          f"certificate stat {cert[:, 0].max():.2e} prim {cert[:, 1].max():.2e}")
    for k in NAMES:
        assert np.isfinite(out[k]).all(), k
        assert errs[k] <= X_TOL, (k, errs[k])
    assert cert.max() <= KKT_TOL, cert.max(axis=0)
    assert (out["b"][~c["mask"]] == 0.0).all()


# ------------------------------------------------------- hand-made masks, every form
def _hand_made(qpb, c, k0, where):
    """The shared H and A are QP k0's of a hand-made case; every QP of the case
    supplies its own mask, x, lam and g.  glam is NaN wherever the call must not
    read it: outside the mask, and on the rows of the mask that the
    orthogonalisation skips on THIS pair (bwd_cases.rows_in_order)."""
    H0, A0 = np.ascontiguousarray(c.H[k0]), np.ascontiguousarray(c.A[k0])
    Bq, m = c.mask.shape
    kept = np.zeros((Bq, m), bool)
    for i in range(Bq):
        kept[i, BC.rows_in_order(H0, A0, c.mask[i])[0]] = True
    gl = np.random.default_rng([SC.SEED, Bq, m, k0, 21]).standard_normal((Bq, m))
    gl[~kept] = np.nan
    act = BC.words(c.mask)
    ref = DP.dual(qpb, BOTH, H0, A0, c.x, c.lam, act, None, c.g, gl)
    F = FB.factor(qpb, H0, A0)
    assert F.result()[1] == OK, where
    got = DP.factored_dual(qpb, F, c.x, c.lam, act, None, c.g, gl)
    DP.same(got, ref, where)
    for k in got:
        assert np.isfinite(got[k]).all(), (where, k)
    if m:
        assert (got["b"][~kept] == 0.0).all(), where
    return kept


@pytest.mark.parametrize("n,m", BC.ALL_ROUTES)
def test_every_form_sizes(qpb, n, m):
    """|W| in {0, 1, n / 2, n - 1, n}."""
    _hand_made(qpb, BC.sizes(n, m), 0, ("sizes", n, m))


@pytest.mark.parametrize("n,m", BC.FORM_ROUTES)
def test_every_form_overfull(qpb, n, m):
    """All m bits set: a row that is a combination of two earlier ones, and the rows met after n independent ones."""
    c = BC.overfull(n, m)
    kept = _hand_made(qpb, c, 0, ("overfull", n, m))
    assert (kept.sum(axis=1) <= n).all() and (~kept & c.mask).any()


@pytest.mark.parametrize("n,m,meq", SHAPES)
def test_a_duplicate_rows_glam_is_ignored(qpb, n, m, meq):
    """Row j2 of the shared A is made a copy of row j1 and marked active wherever
    j1 is: the later of the two is skipped, its glam -- NaN here -- is ignored,
    and gb is 0 there."""
    c = _case(qpb, n, m, meq)
    count = c["mask"].sum(axis=0)
    j1 = int(np.argmax(count))
    j2 = int(np.argmin(np.where(np.arange(m) == j1, B + 1, count)))
    assert count[j1] > 0 and j1 != j2
    A0, lam, mask, gl = c["A0"].copy(), c["lam"].copy(), c["mask"].copy(), c["gl"].copy()
    A0[j2] = A0[j1]
    both = mask[:, j1]
    mask[:, j2] |= both
    lam[both, j2] = 0.37
    gl[both, max(j1, j2)] = np.nan
    gl[~mask] = np.nan
    act = BC.words(mask)
    ref = DP.dual(qpb, BOTH, c["H0"], A0, c["x"], lam, act, c["st"], c["g"], gl)
    F = FB.factor(qpb, c["H0"], A0)
    assert F.result()[1] == OK
    got = DP.factored_dual(qpb, F, c["x"], lam, act, c["st"], c["g"], gl)
    DP.same(got, ref, ("duplicate", j1, j2))
    for k in got:
        assert np.isfinite(got[k]).all(), k
    assert (got["b"][both, max(j1, j2)] == 0.0).all()


# ------------------------------------------------------- NULL outputs, NULL status
@pytest.mark.parametrize("n,m,meq", SHAPES)
def test_every_need_subset_and_null_status(qpb, n, m, meq):
    c = _case(qpb, n, m, meq)
    full = _run(qpb, c)
    DP.same(full, c["ref"], "full")
    for r in range(1, 4):
        for need in itertools.combinations(NAMES, r):
            got = _run(qpb, c, need=need)
            assert set(got) == set(need)
            DP.same(got, {k: full[k] for k in need}, need)
    DP.same(_run(qpb, c, st=None), full, "status NULL")
    sol = qpb.Solution(_dev(c["x"]), _dev(c["lam"]), _dev(c["act"]), None, None)
    F = qpb.factor_shared_backward(_dev(c["H0"]), _dev(c["A0"]))
    gH, gf, gA, gb = qpb.solve_factored_backward_dual(F, sol, _dev(c["g"]), _dev(c["gl"]), need=("f", "b"))
    torch.cuda.synchronize()
    assert gH is None and gA is None
    DP.same({"f": gf.cpu().numpy(), "b": gb.cpu().numpy()}, {"f": full["f"], "b": full["b"]}, "python need")


# ------------------------------------------------------- poisoned QPs
@pytest.mark.parametrize("n,m,meq", SHAPES)
def test_poisoned_qps_contribute_nothing(qpb, n, m, meq):
    c = _case(qpb, n, m, meq)
    bad = np.zeros(B, bool)
    bad[::7] = True
    x, lam, st = c["x"].copy(), c["lam"].copy(), c["st"].copy()
    st[bad] = np.resize([MAX_ITER, NOT_SPD, NUMERICAL], bad.sum())
    x[bad] = np.nan
    lam[bad] = np.nan
    ignored = ~c["mask"] | bad[:, None]
    clean, poisoned = np.where(ignored, 0.0, c["gl"]), np.where(ignored, np.nan, c["gl"])
    ref = DP.dual(qpb, BOTH, c["H0"], c["A0"], x, lam, c["act"], st, c["g"], clean)
    got = _run(qpb, c, x=x, lam=lam, st=st, gl=poisoned)
    DP.same(got, ref, "poison")
    DP.same(_run(qpb, c, x=x, lam=lam, st=st, gl=clean), ref, "clean")
    for k in got:
        assert np.isfinite(got[k]).all(), k
    assert not got["f"][bad].any() and not got["b"][bad].any()


# ------------------------------------------------------- a buffer whose H was not SPD
@pytest.mark.parametrize("n,m,meq", SHAPES)
def test_not_spd(qpb, n, m, meq):
    c = _case(qpb, n, m, meq)
    F = FB.factor(qpb, -np.eye(n), c["A0"])
    assert F.result()[1] == NOT_SPD
    for st in (None, c["st"]):
        got = DP.factored_dual(qpb, F, c["x"], c["lam"], c["act"], st, c["g"], c["gl"])
        assert set(got) == set(NAMES)
        for k in got:
            assert (got[k] == 0).all(), (k, "status NULL" if st is None else "status OK")


# ------------------------------------------------------- streams, reproducibility, the host call
@pytest.mark.parametrize("n,m,meq", SHAPES)
def test_side_stream_and_host_call(qpb, n, m, meq):
    c = _case(qpb, n, m, meq)
    first = _run(qpb, c)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    DP.same(_run(qpb, c, stream=side), first, "side stream")
    qpb.release_stream_workspace(side)
    qpb.release_workspaces()
    DP.same(_run(qpb, c), first, "after release_workspaces")
    hF = qpb.BackwardFactor(c["F"].result()[0], n, m, None)
    hs = qpb.Solution(c["x"], c["lam"], c["act"], c["st"], None)
    got = qpb.solve_factored_backward_dual_host(hF, hs, c["g"], c["gl"])
    DP.same(dict(zip(NAMES, got)), first, "host")
    gH, gf, gA, gb = qpb.solve_factored_backward_dual_host(hF, hs, c["g"], c["gl"], need=("b",))
    assert gH is None and gf is None and gA is None and DP.bits(gb, first["b"])
    plain = qpb.solve_factored_backward_host(hF, hs, c["g"])
    DP.same(dict(zip(NAMES, qpb.solve_factored_backward_dual_host(hF, hs, c["g"], None))), dict(zip(NAMES, plain)),
            "host, glam None")


def test_above_the_wave_class_is_unsupported(qpb):
    import ctypes
    z = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = ctypes.c_void_p(z.data_ptr())
    for n, m in ((33, 0), (16, 65)):
        d = qpb.Desc(n, m, 4, 0, 0, 0.0)
        rc = qpb.lib().qpb_solve_factored_backward_dual(ctypes.byref(d), *([p] * 11), None)
        assert rc == qpb.ERR_UNSUPPORTED, (n, m)
