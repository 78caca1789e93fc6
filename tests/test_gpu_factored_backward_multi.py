"""qpb_solve_factored_backward_multi on the GPU: T right-hand sides (gx, glam)
per QP in one launch on a buffer of qpb_factor_shared_backward -- the MU forms
of the factored forms of both kernels of qpb_kkt_bwd.hip (n <= 16, m <= 32: four
QPs per wavefront, MR = 1 and 2, n == 16 and padded; the rest of n <= 32,
m <= 64: one QP per wavefront), with and without glam.

The reference throughout is the parent's code, which the change does not touch:
qpb_solve_factored_backward_dual (qpb_solve_factored_backward where glam is
NULL) on the same buffer, active and status, once per direction with only the
per-QP outputs asked for, and the comparison is BIT FOR BIT.  One run per kernel
class is held against tests/dual_oracle.py as well, at the project's X_TOL =
1e-6 and KKT_TOL = 1e-9 (tests/bwd_harness.py).

Shapes: shared_cases.SHAPES (both classes, m = 0, n < 16, n = 16, MR = 1 and 2,
the wave class up to (32, 64, meq 8)); B in {1, 5, 67} (67 leaves the
four-per-wave kernels a ragged last wave); T in {1, 2, 5, 17}.  A shape's
forward solve and its 17 single-direction references are computed once per B and
shared: by the contract the first T of them are the reference of a call with T
directions.  The hand-made masks are bwd_cases.sizes and bwd_cases.overfull on
bwd_cases.ALL_ROUTES and FORM_ROUTES, as in tests/test_gpu_factored_backward_dual.py.

Every C call goes into buffers of the test's own, filled with 0xA5 and fenced by
guard words (tests/multi_harness.py).
"""
import numpy as np
import pytest

import bwd_cases as BC
import dual_oracle as DO
import factored_bwd_cases as FB
import multi_harness as MH
import shared_cases as SC
from bwd_harness import KKT_TOL, X_TOL, dev as _dev, rel as _rel

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

OK, MAX_ITER, NOT_SPD, NUMERICAL = 0, 1, 2, 4
BATCHES = (1, 5, 67)
TS = (1, 2, 5, 17)
TMAX = max(TS)
SHAPES = SC.SHAPES
# the parity run against the numpy oracle, one shape per kernel class and load path (every QP of them is OK)
PATH_SHAPES = [(5, 9, 2), (16, 32, 4), (20, 40, 4)]


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    return q


_CASES = {}


def _case(qpb, B, n, m, meq):
    """One shape's shared H0 and A0 at one batch size, its forward on the GPU
    (qpb_solve_shared), TMAX seeded directions, the buffer and the
    single-direction references with and without glam: once, shared, never modified."""
    key = (B, n, m, meq)
    if key not in _CASES:
        H0, f, A0, b = SC.family(B, n, m, meq)
        sol = qpb.solve_shared(_dev(H0), _dev(f), _dev(A0) if m else None, _dev(b) if m else None, meq)
        torch.cuda.synchronize()
        x, lam, act, st = (t.cpu().numpy() for t in (sol.x, sol.lam, sol.active, sol.status))
        if key[1:] in PATH_SHAPES:
            assert (st == OK).all(), st
        rng = np.random.default_rng([SC.SEED, B, n, m, meq, 23])
        g, gl = rng.standard_normal((B, TMAX, n)), rng.standard_normal((B, TMAX, m))
        F = FB.factor(qpb, H0, A0)
        assert F.result()[1] == OK
        ref = MH.factored_single(qpb, F, x, lam, act, st, g, gl if m else None)
        plain = MH.factored_single(qpb, F, x, lam, act, st, g, None) if m else ref
        _CASES[key] = dict(B=B, n=n, m=m, H0=H0, A0=A0, x=x, lam=lam, act=act, st=st, g=g, gl=gl if m else None,
                           ref=ref, plain=plain, F=F,
                           mask=qpb.active_mask_to_bool(act, m) if m else np.zeros((B, 0), bool))
    return _CASES[key]


def _run(qpb, c, T=TMAX, **kw):
    g = kw.pop("g", np.ascontiguousarray(c["g"][:, :T]))
    gl = kw.pop("gl", None if c["gl"] is None else np.ascontiguousarray(c["gl"][:, :T]))
    return MH.factored_multi(qpb, kw.pop("F", c["F"]), kw.pop("act", c["act"]), kw.pop("st", c["st"]), g, gl,
                             kw.pop("B", c["B"]), **kw)


# ------------------------------------------------------- 1. bit for bit against the existing code
@pytest.mark.parametrize("n,m,meq", SHAPES)
def test_every_direction_is_the_single_direction_call(qpb, n, m, meq):
    for B in BATCHES:
        c = _case(qpb, B, n, m, meq)
        for T in TS:
            got = _run(qpb, c, T)
            assert set(got) == ({"f", "b"} if m else {"f"})
            MH.same(got, MH.take(c["ref"], T), (B, T))
            # without glam it is the call without glam
            MH.same(_run(qpb, c, T, gl=None), MH.take(c["plain"], T), (B, T, "glam NULL"))
        if m:
            assert not MH.bits(c["ref"]["f"], c["plain"]["f"])  # the cotangent on lam is not a no-op
        # T = 1 is the existing call's whole output, in its layout
        one = _run(qpb, c, 1)
        for k in one:
            assert MH.bits(one[k][:, 0], np.ascontiguousarray(c["ref"][k][:, 0])), (B, k)


# ------------------------------------------------------- 2. numerics, one shape per kernel class
@pytest.mark.parametrize("n,m,meq", PATH_SHAPES)
def test_parity_and_certificate(qpb, n, m, meq):
    B, T = 67, 5
    c = _case(qpb, B, n, m, meq)
    out = _run(qpb, c, T)
    ref_f, ref_b, cert = np.zeros((B, T, n)), np.zeros((B, T, m)), np.zeros((B, T, 2))
    for i in range(B):
        for t in range(T):
            _, ref_f[i, t], _, ref_b[i, t] = DO.backward(c["H0"], c["x"][i], c["lam"][i], c["A0"], c["mask"][i],
                                                         c["g"][i, t], c["gl"][i, t])
            cert[i, t] = DO.certificate(c["H0"], c["A0"], c["mask"][i], c["g"][i, t], c["gl"][i, t], out["f"][i, t],
                                        out["b"][i, t])
    errs = {"f": max(float(_rel(out["f"][:, t], ref_f[:, t]).max()) for t in range(T)),
            "b": max(float(_rel(out["b"][:, t], ref_b[:, t]).max()) for t in range(T))}
    print(f"({n},{m},{meq}): errors {errs} certificate stat {cert[..., 0].max():.2e} prim {cert[..., 1].max():.2e}")
    assert np.isfinite(out["f"]).all() and np.isfinite(out["b"]).all()
    assert errs["f"] <= X_TOL and errs["b"] <= X_TOL, errs
    assert cert.max() <= KKT_TOL, cert.reshape(-1, 2).max(axis=0)
    assert (out["b"][~np.broadcast_to(c["mask"][:, None, :], out["b"].shape)] == 0.0).all()


# ------------------------------------------------------- 3. directions are independent
@pytest.mark.parametrize("n,m,meq", SHAPES)
def test_directions_are_independent(qpb, n, m, meq):
    B, T = 67, 5
    c = _case(qpb, B, n, m, meq)
    ref = MH.take(c["ref"], T)
    g, gl = np.ascontiguousarray(c["g"][:, :T]), None if not m else np.ascontiguousarray(c["gl"][:, :T])
    # permuting the directions permutes the outputs
    perm = np.array([3, 0, 4, 2, 1])
    got = _run(qpb, c, g=np.ascontiguousarray(g[:, perm]), gl=None if gl is None else np.ascontiguousarray(gl[:, perm]))
    MH.same(got, {k: np.ascontiguousarray(v[:, perm]) for k, v in ref.items()}, "permuted")
    # a NaN-filled direction leaves every other one unchanged
    for s in (0, 2, T - 1):
        gn, gln = g.copy(), None if gl is None else gl.copy()
        gn[:, s] = np.nan
        if gln is not None:
            gln[:, s] = np.nan
        got = _run(qpb, c, g=gn, gl=gln)
        keep = np.arange(T) != s
        MH.same({k: np.ascontiguousarray(v[:, keep]) for k, v in got.items()},
                {k: np.ascontiguousarray(v[:, keep]) for k, v in ref.items()}, ("NaN direction", s))
    # the same direction at t = 0 and at t = T - 1, among 17
    g17, gl17 = c["g"].copy(), None if not m else c["gl"].copy()
    g17[:, TMAX - 1] = g17[:, 0]
    if gl17 is not None:
        gl17[:, TMAX - 1] = gl17[:, 0]
    got = _run(qpb, c, g=g17, gl=gl17)
    for k in got:
        assert MH.bits(np.ascontiguousarray(got[k][:, 0]), np.ascontiguousarray(got[k][:, TMAX - 1])), k
        assert MH.bits(np.ascontiguousarray(got[k][:, 0]), np.ascontiguousarray(c["ref"][k][:, 0])), k


# ------------------------------------------------------- 4. one set of right-hand sides for the batch
@pytest.mark.parametrize("n,m,meq", SHAPES)
def test_shared_rhs_is_the_call_on_copies(qpb, n, m, meq):
    for B in BATCHES:
        c = _case(qpb, B, n, m, meq)
        for T in (1, 5, 17):
            g0 = np.ascontiguousarray(c["g"][0, :T])
            gl0 = None if not m else np.ascontiguousarray(c["gl"][0, :T])
            got = _run(qpb, c, g=g0, gl=gl0)
            assert got["f"].shape == (B, T, n)
            ref = _run(qpb, c, g=SC.expand(g0, B), gl=None if gl0 is None else SC.expand(gl0, B))
            MH.same(got, ref, (B, T, "shared rhs"))
            MH.same(_run(qpb, c, g=g0, gl=None), _run(qpb, c, g=SC.expand(g0, B), gl=None), (B, T, "shared, no glam"))


# ------------------------------------------------------- 5. edge cases, each against the single-direction call
T_EDGE = 5


def _hand_made(qpb, c, k0, where):
    """The shared H and A are QP k0's of a hand-made case; every QP of the case
    supplies its own mask.  glam is NaN wherever the call must not read it:
    outside the mask, and on the rows of the mask that the orthogonalisation
    skips on THIS pair (bwd_cases.rows_in_order)."""
    H0, A0 = np.ascontiguousarray(c.H[k0]), np.ascontiguousarray(c.A[k0])
    Bq, m = c.mask.shape
    n = H0.shape[0]
    kept = np.zeros((Bq, m), bool)
    for i in range(Bq):
        kept[i, BC.rows_in_order(H0, A0, c.mask[i])[0]] = True
    rng = np.random.default_rng([SC.SEED, Bq, m, k0, 24])
    g, gl = rng.standard_normal((Bq, T_EDGE, n)), rng.standard_normal((Bq, T_EDGE, m))
    drop = np.broadcast_to(~kept[:, None, :], gl.shape)
    gl[drop] = np.nan
    act = BC.words(c.mask)
    F = FB.factor(qpb, H0, A0)
    assert F.result()[1] == OK, where
    ref = MH.factored_single(qpb, F, c.x, c.lam, act, None, g, gl if m else None)
    got = MH.factored_multi(qpb, F, act, None, g, gl if m else None, Bq)
    MH.same(got, ref, where)
    for k in got:
        assert np.isfinite(got[k]).all(), (where, k)
    if m:
        assert (got["b"][drop] == 0.0).all(), where
    return kept


@pytest.mark.parametrize("n,m", BC.ALL_ROUTES)
def test_every_form_sizes(qpb, n, m):
    """|W| in {0, 1, n / 2, n - 1, n}."""
    _hand_made(qpb, BC.sizes(n, m), 0, ("sizes", n, m))


@pytest.mark.parametrize("n,m", BC.FORM_ROUTES)
def test_every_form_overfull(qpb, n, m):
    """All m bits set: a dependent row, and the rows met after n independent ones."""
    c = BC.overfull(n, m)
    kept = _hand_made(qpb, c, 0, ("overfull", n, m))
    assert (kept.sum(axis=1) <= n).all() and (~kept & c.mask).any()


@pytest.mark.parametrize("n,m", BC.COND_SHAPES)
def test_ill_conditioned_h(qpb, n, m):
    """cond(H) = 1e10: the H and A of the family's QP with |W| = n, every QP's mask."""
    H, A, mask, x, lam, g1, p, size = BC.conditioned_inputs(n, m)
    k0 = int(np.flatnonzero((p == 10) & (size == size.max()))[0])
    H0, A0 = np.ascontiguousarray(H[k0]), np.ascontiguousarray(A[k0])
    Bq = len(H)
    rng = np.random.default_rng([SC.SEED, n, m, 25])
    g, gl = rng.standard_normal((Bq, T_EDGE, n)), rng.standard_normal((Bq, T_EDGE, m))
    g[:, 0] = g1
    act = BC.words(mask)
    F = FB.factor(qpb, H0, A0)
    assert F.result()[1] == OK
    ref = MH.factored_single(qpb, F, x, lam, act, None, g, gl)
    MH.same(MH.factored_multi(qpb, F, act, None, g, gl, Bq), ref, ("cond 1e10", n, m))
    assert np.isfinite(ref["f"]).all()


@pytest.mark.parametrize("n,m,meq", [s for s in SHAPES if s[1] % 32])  # (the others' words have no position past m)
def test_bits_past_m_are_ignored(qpb, n, m, meq):
    B, T = 5, 2
    c = _case(qpb, B, n, m, meq)
    act = c["act"].view(np.uint32).copy()
    act[:, -1] |= np.uint32((0xFFFFFFFF << (m % 32)) & 0xFFFFFFFF)
    MH.same(_run(qpb, c, T, act=act.view(np.int32)), MH.take(c["ref"], T), "bits past m")


@pytest.mark.parametrize("n,m,meq", SHAPES)
def test_poisoned_qps_get_zeros_in_every_direction(qpb, n, m, meq):
    B, T = 67, 5
    c = _case(qpb, B, n, m, meq)
    bad = np.zeros(B, bool)
    bad[::7] = True
    st = c["st"].copy()
    st[bad] = np.resize([MAX_ITER, NOT_SPD, NUMERICAL], bad.sum())
    g = np.ascontiguousarray(c["g"][:, :T])
    g[bad] = np.nan
    gl = None
    if m:
        gl = np.where((~c["mask"] | bad[:, None])[:, None, :], np.nan, c["gl"][:, :T])
    got = _run(qpb, c, st=st, g=g, gl=gl)
    ref = MH.take(c["ref"], T)
    for k in got:
        assert np.isfinite(got[k]).all(), k
        assert not got[k][bad].any(), k
        ok = ~bad & (c["st"] == OK)
        assert MH.bits(np.ascontiguousarray(got[k][ok]), np.ascontiguousarray(ref[k][ok])), k
    # ... and bit for bit the single-direction call on the same inputs
    x, lam = c["x"].copy(), c["lam"].copy()
    x[bad] = np.nan
    lam[bad] = np.nan
    MH.same(got, MH.factored_single(qpb, c["F"], x, lam, c["act"], st, g, gl), "poisoned")


@pytest.mark.parametrize("n,m,meq", SHAPES)
def test_not_spd_buffer_gives_zeros(qpb, n, m, meq):
    B, T = 5, 5
    c = _case(qpb, B, n, m, meq)
    F = FB.factor(qpb, -np.eye(n), c["A0"])
    assert F.result()[1] == NOT_SPD
    for st in (None, c["st"]):
        got = _run(qpb, c, T, F=F, st=st)
        assert set(got) == ({"f", "b"} if m else {"f"})
        for k in got:
            assert (got[k] == 0).all(), (k, "status NULL" if st is None else "status given")


# ------------------------------------------------------- 6. call mechanics
@pytest.mark.parametrize("n,m,meq", SHAPES)
def test_every_need_subset_and_null_status(qpb, n, m, meq):
    B, T = 67, 5
    c = _case(qpb, B, n, m, meq)
    full = _run(qpb, c, T)
    for need in (("f",), ("b",), ("f", "b")):
        if not m and need == ("b",):
            continue  # gb is ignored at m == 0: no output left
        got = _run(qpb, c, T, need=need)
        assert set(got) == set(need) & set(full)
        MH.same(got, {k: full[k] for k in got}, need)
    # status NULL counts as OK
    st_ok = np.zeros_like(c["st"])
    MH.same(_run(qpb, c, T, st=None), _run(qpb, c, T, st=st_ok), "status NULL")


@pytest.mark.parametrize("n,m,meq", SHAPES)
def test_a_qp_depends_on_its_own_inputs_only(qpb, n, m, meq):
    """A QP's bits at two batch positions and sizes."""
    B, T = 67, 5
    c = _case(qpb, B, n, m, meq)
    full = MH.take(c["ref"], T)
    g, gl = c["g"][:, :T], None if not m else c["gl"][:, :T]
    pick = lambda idx, a: None if a is None else np.ascontiguousarray(a[idx])  # noqa: E731
    for idx in (np.array([5]), np.random.default_rng(SC.SEED).permutation(B)[:31]):
        got = _run(qpb, c, B=len(idx), act=pick(idx, c["act"]), st=pick(idx, c["st"]), g=pick(idx, g), gl=pick(idx, gl))
        MH.same(got, {k: pick(idx, v) for k, v in full.items()}, ("moved", len(idx)))


@pytest.mark.parametrize("n,m,meq", SHAPES)
def test_side_stream_host_and_python_calls(qpb, n, m, meq):
    B, T = 67, 5
    c = _case(qpb, B, n, m, meq)
    full = MH.take(c["ref"], T)
    g, gl = np.ascontiguousarray(c["g"][:, :T]), None if not m else np.ascontiguousarray(c["gl"][:, :T])
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    MH.same(_run(qpb, c, T, stream=side), full, "side stream")
    # the host call
    hF = qpb.BackwardFactor(c["F"].result()[0], n, m, None)
    hs = qpb.Solution(None, None, c["act"] if m else None, c["st"], None)
    gf, gb = qpb.solve_factored_backward_multi_host(hF, hs, g, gl)
    MH.same({k: v for k, v in (("f", gf), ("b", gb)) if v is not None}, full, "host")
    gf, gb = qpb.solve_factored_backward_multi_host(hF, hs, g[0], None if gl is None else gl[0], need=("f",))
    assert gb is None and MH.bits(gf, _run(qpb, c, g=np.ascontiguousarray(g[0]),
                                           gl=None if gl is None else np.ascontiguousarray(gl[0]))["f"])
    # the Python call, on the device and on a stream
    F = qpb.factor_shared_backward(_dev(c["H0"]), _dev(c["A0"]) if m else None)
    sol = qpb.Solution(_dev(c["x"]), _dev(c["lam"]) if m else None, _dev(c["act"]) if m else None, _dev(c["st"]), None)
    dgl = None if gl is None else _dev(gl)
    gf, gb = qpb.solve_factored_backward_multi(F, sol, _dev(g), dgl)
    torch.cuda.synchronize()
    MH.same({k: v.cpu().numpy() for k, v in (("f", gf), ("b", gb)) if v is not None}, full, "python")
    with torch.cuda.stream(side):
        gf, gb = qpb.solve_factored_backward_multi(F, sol, _dev(g), dgl, need=("f",), stream=side)
    side.synchronize()
    assert gb is None and MH.bits(gf.cpu().numpy(), full["f"])
    # the tangents wrapper is solve_factored_tangent per direction
    db = None if gl is None else _dev(-gl)
    dx, dlam = qpb.solve_factored_tangents(F, sol, _dev(g), db)
    torch.cuda.synchronize()
    for t in range(T):
        dx1, dl1 = qpb.solve_factored_tangent(F, sol, _dev(np.ascontiguousarray(g[:, t])),
                                              None if db is None else db[:, t].contiguous())
        torch.cuda.synchronize()
        assert MH.bits(dx[:, t].cpu().numpy(), dx1.cpu().numpy()), t
        assert (dlam is None and dl1 is None) or MH.bits(dlam[:, t].cpu().numpy(), dl1.cpu().numpy()), t


def test_above_the_wave_class_is_unsupported(qpb):
    import ctypes
    z = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = ctypes.c_void_p(z.data_ptr())
    for n, m in ((33, 0), (16, 65)):
        d = qpb.Desc(n, m, 4, 0, 0, 0.0)
        rc = qpb.lib().qpb_solve_factored_backward_multi(ctypes.byref(d), p, p, p, 2, 0, p, p, p, p, None)
        assert rc == qpb.ERR_UNSUPPORTED, (n, m)


# ------------------------------------------------------- 7. the Jacobian dx* / df from gx = I
@pytest.mark.parametrize("n,m,meq", PATH_SHAPES + [(3, 0, 0), (32, 64, 8)])
def test_jacobian_from_identity_directions(qpb, n, m, meq):
    """gx = I shared (T = n), no glam: gf[k] as an n x n matrix is dx* / df (up to
    the sign of the right-hand side), symmetric, and A_W times it vanishes."""
    B = 67
    c = _case(qpb, B, n, m, meq)
    J = _run(qpb, c, g=np.eye(n), gl=None, need=("f",))["f"]  # (B, T = n, n): row t is dx for gx = e_t
    assert J.shape == (B, n, n) and np.isfinite(J).all()
    ok = c["st"] == OK
    assert ok.sum() > B // 2
    sym = _rel(J[ok], J[ok].transpose(0, 2, 1))
    print(f"({n},{m},{meq}): asymmetry {sym.max():.2e}")
    assert sym.max() <= X_TOL
    if m:
        An = np.abs(c["A0"]).sum(axis=1).max()
        worst = 0.0
        for i in np.flatnonzero(ok):
            W = np.flatnonzero(c["mask"][i])
            if len(W):
                # dual_oracle.certificate's primal measure with glam = 0, per direction
                r = np.abs(c["A0"][W] @ J[i].T).max(axis=0) / (1.0 + An * np.abs(J[i]).max(axis=1))
                worst = max(worst, float(r.max()))
        print(f"({n},{m},{meq}): |A_W J| {worst:.2e}")
        assert worst <= KKT_TOL
