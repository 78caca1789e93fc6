"""qpb_solve_box_backward_multi on the GPU: T right-hand sides (gx, glam) per
box QP in one launch -- the MU forms of both kernels of qpb_kkt_bwd_box.hip
(n <= 16: four QPs per wavefront, n < 16 and n == 16; 16 < n <= 32: one QP per
wavefront), with a batched H and with one H, with and without glam.

The reference throughout is the parent's code, which the change does not touch:
qpb_solve_box_backward_dual (the box backward where glam is NULL) on the same H,
shared & QPB_SHARED_H, active and status, once per direction with only the
per-QP outputs asked for, and the comparison is BIT FOR BIT.  Each direction is
held to tests/box_dual_oracle.py as well, at the project's X_TOL = 1e-6 and
KKT_TOL = 1e-9 (tests/bwd_harness.py).

Shapes: n in {1, 5, 16, 17, 20, 32}; B in {1, 5, 67} (67 leaves the
four-per-wave kernel a ragged last wave); T in {1, 2, 5, 17}.  The forward is
qpb.solve_box on box_bwd_oracle.cycled(11, B, n) (widths 10, 1 and 0.1: from few
fixed variables to all of them).  A shape's forward and its 17 single-direction
references are computed once per B and shared: by the contract the first T of
them are the reference of a call with T directions.

Every C call goes into buffers of the test's own, filled with 0xA5 and fenced by
guard words (tests/multi_harness.py).
"""
import itertools

import numpy as np
import pytest

import box_bwd_oracle as BO
import box_dual_oracle as BD
import bwd_cases as BC
import dual_oracle as DO
import multi_harness as MH
import shared_cases as SC
from bwd_harness import KKT_TOL, X_TOL, dev as _dev, rel as _rel
from multi_harness import BOX_NAMES as NAMES, SHARED_H

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

OK, MAX_ITER, NOT_SPD, NUMERICAL = 0, 1, 2, 4
SEED = 11
BATCHES = (1, 5, 67)
TS = (1, 2, 5, 17)
TMAX = max(TS)
SHAPES = [1, 5, 16, 17, 20, 32]


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    return q


_CASES = {}


def _case(qpb, B, n):
    """One shape's inputs at one batch size, its forward on the GPU, TMAX seeded
    directions and the single-direction references (per-QP H and one H, with
    and without glam): computed once, shared, never modified."""
    if (B, n) not in _CASES:
        H, f, lb, ub, _ = BO.cycled(SEED, B, n)
        sol = qpb.solve_box(_dev(H), _dev(f), _dev(lb), _dev(ub))
        torch.cuda.synchronize()
        x, act, st = (t.cpu().numpy() for t in (sol.x, sol.active, sol.status))
        assert (st == OK).all(), st
        rng = np.random.default_rng([SEED, B, n, 26])
        g, gl = rng.standard_normal((B, TMAX, n)), rng.standard_normal((B, TMAX, 2 * n))
        H0 = np.ascontiguousarray(H[0])
        _CASES[(B, n)] = dict(B=B, n=n, H=H, H0=H0, x=x, act=act, st=st, g=g, gl=gl,
                              mask=qpb.active_mask_to_bool(act, 2 * n),
                              ref=MH.box_single(qpb, 0, H, x, act, st, g, gl),
                              plain=MH.box_single(qpb, 0, H, x, act, st, g, None),
                              ref0=MH.box_single(qpb, SHARED_H, H0, x, act, st, g, gl),
                              plain0=MH.box_single(qpb, SHARED_H, H0, x, act, st, g, None))
    return _CASES[(B, n)]


def _run(qpb, c, T=TMAX, **kw):
    shared = kw.pop("shared", 0)
    g = kw.pop("g", np.ascontiguousarray(c["g"][:, :T]))
    gl = kw.pop("gl", np.ascontiguousarray(c["gl"][:, :T]))
    return MH.box_multi(qpb, shared, kw.pop("H", c["H0"] if shared else c["H"]), kw.pop("act", c["act"]),
                        kw.pop("st", c["st"]), g, gl, kw.pop("B", c["B"]), **kw)


# ------------------------------------------------------- 1. bit for bit against the existing code
@pytest.mark.parametrize("n", SHAPES)
def test_every_direction_is_the_single_direction_call(qpb, n):
    for B in BATCHES:
        c = _case(qpb, B, n)
        for T in TS:
            for shared, ref, plain in ((0, c["ref"], c["plain"]), (SHARED_H, c["ref0"], c["plain0"])):
                got = _run(qpb, c, T, shared=shared)
                assert set(got) == set(NAMES)
                MH.same(got, MH.take(ref, T), (B, T, shared))
                # without glam it is the box backward
                MH.same(_run(qpb, c, T, shared=shared, gl=None), MH.take(plain, T), (B, T, shared, "glam NULL"))
        # T = 1 is the existing call's whole output, in its layout
        one = _run(qpb, c, 1)
        for k in one:
            assert MH.bits(one[k][:, 0], np.ascontiguousarray(c["ref"][k][:, 0])), (B, k)
    c = _case(qpb, 67, n)
    assert not MH.bits(c["ref"]["f"], c["plain"]["f"])  # the cotangent on lam is not a no-op
    # one H is QP 0's H: QP 0's outputs are those of the batched call
    for k in NAMES:
        assert MH.bits(np.ascontiguousarray(c["ref0"][k][0]), np.ascontiguousarray(c["ref"][k][0])), k


# ------------------------------------------------------- 2. numerics: every direction against the oracle
@pytest.mark.parametrize("n", SHAPES)
def test_parity_and_certificate(qpb, n):
    B, T = 67, 5
    c = _case(qpb, B, n)
    out = _run(qpb, c, T)
    A = BO.dense(np.zeros((1, n)), np.zeros((1, n)))[0][0]
    dm = BO.dense_mask(c["mask"])
    fixed = c["mask"][:, :n] | c["mask"][:, n:]
    count = fixed.sum(axis=1)
    assert count.max() == n and count.min() <= n // 2  # from few fixed variables to all of them
    errs, cert = {k: 0.0 for k in NAMES}, np.zeros((B, T, 2))
    for t in range(T):
        ref = BD.backward_batch(c["H"], c["x"], c["mask"], c["g"][:, t], c["gl"][:, t])
        for k in NAMES:
            errs[k] = max(errs[k], float(_rel(out[k][:, t], ref[k]).max()))
        gb = BO.to_gb(out["ub"][:, t], out["lb"][:, t])
        for i in range(B):
            cert[i, t] = DO.certificate(c["H"][i], A, dm[i], c["g"][i, t], c["gl"][i, t], out["f"][i, t], gb[i])
        # dx is -glam or +glam on the fixed variables, exactly
        d = np.array([BD.prescribed(c["mask"][i], c["gl"][i, t]) for i in range(B)])
        assert np.array_equal(out["f"][:, t][fixed], d[fixed]), t
        assert (out["ub"][:, t][~c["mask"][:, :n]] == 0.0).all() and (out["lb"][:, t][~c["mask"][:, n:]] == 0.0).all()
    print(f"n={n}: errors {errs} certificate stat {cert[..., 0].max():.2e} prim {cert[..., 1].max():.2e}")
    for k in NAMES:
        assert np.isfinite(out[k]).all(), k
        assert errs[k] <= X_TOL, (k, errs[k])
    assert cert.max() <= KKT_TOL, cert.reshape(-1, 2).max(axis=0)


# ------------------------------------------------------- 3. directions are independent
@pytest.mark.parametrize("n", SHAPES)
def test_directions_are_independent(qpb, n):
    B, T = 67, 5
    c = _case(qpb, B, n)
    ref = MH.take(c["ref"], T)
    g, gl = np.ascontiguousarray(c["g"][:, :T]), np.ascontiguousarray(c["gl"][:, :T])
    perm = np.array([3, 0, 4, 2, 1])
    got = _run(qpb, c, g=np.ascontiguousarray(g[:, perm]), gl=np.ascontiguousarray(gl[:, perm]))
    MH.same(got, {k: np.ascontiguousarray(v[:, perm]) for k, v in ref.items()}, "permuted")
    for s in (0, 2, T - 1):
        gn, gln = g.copy(), gl.copy()
        gn[:, s] = np.nan
        gln[:, s] = np.nan
        got = _run(qpb, c, g=gn, gl=gln)
        keep = np.arange(T) != s
        MH.same({k: np.ascontiguousarray(v[:, keep]) for k, v in got.items()},
                {k: np.ascontiguousarray(v[:, keep]) for k, v in ref.items()}, ("NaN direction", s))
    g17, gl17 = c["g"].copy(), c["gl"].copy()
    g17[:, TMAX - 1], gl17[:, TMAX - 1] = g17[:, 0], gl17[:, 0]
    got = _run(qpb, c, g=g17, gl=gl17)
    for k in got:
        assert MH.bits(np.ascontiguousarray(got[k][:, 0]), np.ascontiguousarray(got[k][:, TMAX - 1])), k
        assert MH.bits(np.ascontiguousarray(got[k][:, 0]), np.ascontiguousarray(c["ref"][k][:, 0])), k


# ------------------------------------------------------- 4. one set of right-hand sides for the batch
@pytest.mark.parametrize("n", SHAPES)
def test_shared_rhs_is_the_call_on_copies(qpb, n):
    for B in BATCHES:
        c = _case(qpb, B, n)
        for T in (1, 5, 17):
            g0, gl0 = np.ascontiguousarray(c["g"][0, :T]), np.ascontiguousarray(c["gl"][0, :T])
            for shared in (0, SHARED_H):  # QPB_SHARED_H combined with QPB_SHARED_RHS included
                got = _run(qpb, c, shared=shared, g=g0, gl=gl0)
                assert got["f"].shape == (B, T, n)
                MH.same(got, _run(qpb, c, shared=shared, g=SC.expand(g0, B), gl=SC.expand(gl0, B)), (B, T, shared))
                MH.same(_run(qpb, c, shared=shared, g=g0, gl=None),
                        _run(qpb, c, shared=shared, g=SC.expand(g0, B), gl=None), (B, T, shared, "no glam"))


# ------------------------------------------------------- 5. edge cases, each against the single-direction call
HAND, T_EDGE = 8, 5


def _hand(qpb, n):
    c = _case(qpb, 67, n)
    s = slice(0, HAND)
    return (c, c["H"][s], c["x"][s], c["st"][s], np.ascontiguousarray(c["g"][s, :T_EDGE]), c["mask"][s],
            np.ascontiguousarray(c["gl"][s, :T_EDGE]))


def _edge(qpb, H, x, mask, st, g, gl, where):
    act = BC.words(mask)
    got = MH.box_multi(qpb, 0, H, act, st, g, gl, len(H))
    MH.same(got, MH.box_single(qpb, 0, H, x, act, st, g, gl), where)
    for k in got:
        assert np.isfinite(got[k]).all(), (where, k)
    return got


@pytest.mark.parametrize("n", SHAPES)
def test_both_bits_of_a_variable_set(qpb, n):
    """The upper bound counts: dx = -glam of the upper entry, the lower entry's
    glam -- NaN here -- is ignored and glb = 0."""
    c, H, x, st, g, mask, gl = _hand(qpb, n)
    mask, gl = mask.copy(), gl.copy()
    rows = np.arange(HAND)
    var = rows * 3 % n
    mask[rows, var] = True
    mask[rows, n + var] = True
    gl[rows, :, n + var] = np.nan
    out = _edge(qpb, H, x, mask, st, g, gl, "both bits")
    assert (out["lb"][rows, :, var] == 0.0).all()
    assert np.array_equal(out["f"][rows, :, var], -gl[rows, :, var])


@pytest.mark.parametrize("n", SHAPES)
def test_all_bits_and_no_bit_set(qpb, n):
    c, H, x, st, g, _, gl = _hand(qpb, n)
    up = gl.copy()
    up[:, :, n:] = np.nan
    out = _edge(qpb, H, x, np.ones((HAND, 2 * n), bool), st, g, up, "all bits")
    assert np.array_equal(out["f"], -up[:, :, :n]) and (out["lb"] == 0.0).all()
    low = np.zeros((HAND, 2 * n), bool)
    low[:, n:] = True
    lo = gl.copy()
    lo[:, :, :n] = np.nan
    out = _edge(qpb, H, x, low, st, g, lo, "all lower bits")
    assert np.array_equal(out["f"], lo[:, :, n:]) and (out["ub"] == 0.0).all()
    # none fixed: glam -- all NaN -- is wholly ignored
    none = np.zeros((HAND, 2 * n), bool)
    out = _edge(qpb, H, x, none, st, g, np.full_like(gl, np.nan), "no bit")
    MH.same(out, MH.box_single(qpb, 0, H, x, BC.words(none), st, g, None), "no bit, glam NULL")
    assert (out["lb"] == 0.0).all() and (out["ub"] == 0.0).all()


@pytest.mark.parametrize("n", [1, 5, 17, 20])  # (n = 16 and 32 fill their words: no position >= 2n)
def test_bits_past_2n_are_ignored(qpb, n):
    c, H, x, st, g, mask, gl = _hand(qpb, n)
    act = BC.words(mask)
    nan_gl = np.where(mask[:, None, :], gl, np.nan)  # NaN at every clear bit
    last = act.view(np.uint32).copy()
    spare = np.uint32((0xFFFFFFFF << ((2 * n) % 32)) & 0xFFFFFFFF)
    last[:, -1] |= spare & np.uint32(0xDEADBEEF | (1 << 31) | (1 << ((2 * n) % 32)))
    assert (last[:, -1] != act.view(np.uint32)[:, -1]).all()
    got = MH.box_multi(qpb, 0, H, last.view(np.int32), st, g, nan_gl, HAND)
    MH.same(got, {k: np.ascontiguousarray(v[:HAND, :T_EDGE]) for k, v in c["ref"].items()}, "bits past 2n")


@pytest.mark.parametrize("n", [16, 32])
def test_ill_conditioned_h(qpb, n):
    """cond(H) = 1e10 (bwd_cases.conditioned_inputs, its H only), about a third of
    the variables fixed and all but one, at the upper or the lower bound at random."""
    Hs, *_, ps, _ = BC.conditioned_inputs(n, 2 * n)
    rs = np.random.default_rng([131, n, 27])
    H, mask = [], []
    for Hq in Hs[ps == 10]:
        for kd in ("third", "all_but_one"):
            fixed = rs.permutation(n)[:n // 3] if kd == "third" else np.delete(np.arange(n), rs.integers(n))
            mk = np.zeros(2 * n, bool)
            mk[fixed + n * (rs.random(len(fixed)) < 0.5)] = True
            H.append(Hq)
            mask.append(mk)
    H, mask = np.array(H), np.array(mask)
    Bq = len(H)
    assert Bq == 10
    x, g, gl = rs.standard_normal((Bq, n)), rs.standard_normal((Bq, T_EDGE, n)), rs.standard_normal((Bq, T_EDGE, 2 * n))
    out = _edge(qpb, H, x, mask, None, g, gl, "cond 1e10")
    fixed = mask[:, :n] | mask[:, n:]
    for t in range(T_EDGE):
        d = np.array([BD.prescribed(mask[i], gl[i, t]) for i in range(Bq)])
        assert np.array_equal(out["f"][:, t][fixed], d[fixed])


@pytest.mark.parametrize("n", SHAPES)
def test_poisoned_qps_get_zeros_in_every_direction(qpb, n):
    B, T = 67, 5
    c = _case(qpb, B, n)
    bad = np.zeros(B, bool)
    bad[::7] = True
    st = c["st"].copy()
    st[bad] = np.resize([MAX_ITER, NOT_SPD, NUMERICAL], bad.sum())
    g = np.ascontiguousarray(c["g"][:, :T])
    g[bad] = np.nan
    ignored = ~BO.dense_mask(c["mask"]) | bad[:, None]
    gl = np.where(ignored[:, None, :], np.nan, c["gl"][:, :T])
    for shared, ref in ((0, c["ref"]), (SHARED_H, c["ref0"])):
        got = _run(qpb, c, shared=shared, st=st, g=g, gl=gl)
        for k in NAMES:
            assert np.isfinite(got[k]).all(), k
            assert (got[k][bad] == 0.0).all(), k
            assert MH.bits(np.ascontiguousarray(got[k][~bad]), np.ascontiguousarray(ref[k][~bad, :T])), k


# ------------------------------------------------------- 6. call mechanics
@pytest.mark.parametrize("n", SHAPES)
def test_every_need_subset_and_null_status(qpb, n):
    B, T = 67, 5
    c = _case(qpb, B, n)
    full = MH.take(c["ref"], T)
    for r in range(1, 4):
        for need in itertools.combinations(NAMES, r):
            got = _run(qpb, c, T, need=need)
            assert set(got) == set(need)
            MH.same(got, {k: full[k] for k in need}, need)
    MH.same(_run(qpb, c, T, st=None), full, "status NULL")  # (every QP of the case is OK)
    MH.same(_run(qpb, c, T, shared=SHARED_H, st=None, need=("ub",)), {"ub": MH.take(c["ref0"], T)["ub"]}, "one H")


@pytest.mark.parametrize("n", SHAPES)
def test_a_qp_depends_on_its_own_inputs_only(qpb, n):
    """A QP's bits at two batch positions and sizes, and with its neighbours poisoned."""
    B, T = 67, 5
    c = _case(qpb, B, n)
    full = MH.take(c["ref"], T)
    g, gl = c["g"][:, :T], c["gl"][:, :T]
    pick = lambda idx, a: np.ascontiguousarray(a[idx])  # noqa: E731
    for idx in (np.array([5]), np.random.default_rng(SEED).permutation(B)[:31]):
        got = _run(qpb, c, B=len(idx), H=pick(idx, c["H"]), act=pick(idx, c["act"]), st=pick(idx, c["st"]),
                   g=pick(idx, g), gl=pick(idx, gl))
        MH.same(got, {k: pick(idx, v) for k, v in full.items()}, ("moved", len(idx)))
    k = 5
    arrays = {j: np.array(v) for j, v in (("H", c["H"]), ("g", g), ("gl", gl))}
    others = np.arange(B) != k
    for v in arrays.values():
        v[others] = np.nan
    poisoned = _run(qpb, c, H=arrays["H"], g=arrays["g"], gl=arrays["gl"])
    MH.same({j: v[k:k + 1] for j, v in poisoned.items()}, {j: v[k:k + 1] for j, v in full.items()}, "neighbours poisoned")


@pytest.mark.parametrize("n", SHAPES)
def test_side_stream_host_and_python_calls(qpb, n):
    B, T = 67, 5
    c = _case(qpb, B, n)
    full, full0 = MH.take(c["ref"], T), MH.take(c["ref0"], T)
    g, gl = np.ascontiguousarray(c["g"][:, :T]), np.ascontiguousarray(c["gl"][:, :T])
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    MH.same(_run(qpb, c, T, stream=side), full, "side stream")
    # the host call: per-QP H, one H, one set of right-hand sides, glam None
    hs = qpb.Solution(None, None, c["act"], c["st"], None)
    MH.same(dict(zip(NAMES, qpb.solve_box_backward_multi_host(c["H"], hs, g, gl))), full, "host")
    MH.same(dict(zip(NAMES, qpb.solve_box_backward_multi_host(c["H0"], hs, g, gl))), full0, "host, one H")
    MH.same(dict(zip(NAMES, qpb.solve_box_backward_multi_host(c["H0"], hs, g[0], gl[0]))),
            _run(qpb, c, shared=SHARED_H, g=np.ascontiguousarray(g[0]), gl=np.ascontiguousarray(gl[0])), "host, shared")
    gf, glb, gub = qpb.solve_box_backward_multi_host(c["H"], hs, g, None, need=("lb",))
    assert gf is None and gub is None and MH.bits(glb, MH.take(c["plain"], T)["lb"])
    # the Python call, on the device and on a stream
    sol = qpb.Solution(_dev(c["x"]), None, _dev(c["act"]), _dev(c["st"]), None)
    out = qpb.solve_box_backward_multi(_dev(c["H"]), sol, _dev(g), _dev(gl))
    torch.cuda.synchronize()
    MH.same({k: t.cpu().numpy() for k, t in zip(NAMES, out)}, full, "python")
    with torch.cuda.stream(side):
        gf, glb, gub = qpb.solve_box_backward_multi(_dev(c["H0"]), sol, _dev(g), _dev(gl), need=("f", "ub"), stream=side)
    side.synchronize()
    assert glb is None
    MH.same({"f": gf.cpu().numpy(), "ub": gub.cpu().numpy()}, {"f": full0["f"], "ub": full0["ub"]}, "python, one H")
    # the tangents wrapper is solve_box_tangent per direction
    rng = np.random.default_rng([SEED, n, 28])
    dlb, dub = _dev(rng.standard_normal((B, T, n))), _dev(rng.standard_normal((B, T, n)))
    for Hd in (_dev(c["H"]), _dev(c["H0"])):
        for lo, hi in ((dlb, dub), (None, dub), (None, None)):
            dx, dlam = qpb.solve_box_tangents(Hd, sol, _dev(g), lo, hi)
            torch.cuda.synchronize()
            assert dx.shape == (B, T, n) and dlam.shape == (B, T, 2 * n)
            for t in (0, T - 1):
                dx1, dl1 = qpb.solve_box_tangent(Hd, sol, _dev(np.ascontiguousarray(g[:, t])),
                                                 None if lo is None else lo[:, t].contiguous(),
                                                 None if hi is None else hi[:, t].contiguous())
                torch.cuda.synchronize()
                assert MH.bits(dx[:, t].cpu().numpy(), dx1.cpu().numpy()), t
                assert MH.bits(dlam[:, t].cpu().numpy(), dl1.cpu().numpy()), t


def test_above_the_wave_class_is_unsupported(qpb):
    n, Bq, T = 33, 2, 3
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")  # noqa: E731
    act = torch.zeros((Bq, (2 * n + 31) // 32), dtype=torch.int32, device="cuda")
    sol = qpb.Solution(None, None, act, None, None)
    with pytest.raises(qpb.QPBError) as e:
        qpb.solve_box_backward_multi(z(Bq, n, n), sol, z(Bq, T, n), z(Bq, T, 2 * n))
    assert e.value.code == qpb.ERR_UNSUPPORTED and "n<=32" in str(e.value)


# ------------------------------------------------------- 7. the Jacobian dx* / df from gx = I
@pytest.mark.parametrize("n", SHAPES)
def test_jacobian_from_identity_directions(qpb, n):
    """gx = I shared (T = n), no glam: gf[k] as an n x n matrix is dx* / df (up to
    the sign of the right-hand side): symmetric, and its rows and columns of the
    fixed variables -- A_W times it, on unit rows -- vanish."""
    B = 67
    c = _case(qpb, B, n)
    J = _run(qpb, c, g=np.eye(n), gl=None, need=("f",))["f"]
    assert J.shape == (B, n, n) and np.isfinite(J).all()
    sym = _rel(J, J.transpose(0, 2, 1))
    print(f"n={n}: asymmetry {sym.max():.2e}")
    assert sym.max() <= X_TOL
    fixed = c["mask"][:, :n] | c["mask"][:, n:]
    worst = 0.0
    for i in range(B):
        W = np.flatnonzero(fixed[i])
        if len(W):
            # dual_oracle.certificate's primal measure with glam = 0 and ||A||_inf = 1, per direction
            r = np.abs(J[i][:, W]).max(axis=1) / (1.0 + np.abs(J[i]).max(axis=1))
            worst = max(worst, float(r.max()))
    print(f"n={n}: |A_W J| {worst:.2e}")
    assert worst <= KKT_TOL
