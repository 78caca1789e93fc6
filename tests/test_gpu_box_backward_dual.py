"""qpb_solve_box_backward_dual on the GPU: the gradients of a box solve for a
loss that reads the multipliers too, in the DU forms of both kernels of
qpb_kkt_bwd_box.hip (n <= 16: four QPs per wavefront, n < 16 and n == 16;
16 < n <= 32: one QP per wavefront), with a batched H and with one H.

The forward is qpb.solve_box on the GPU (box_bwd_oracle.cycled(11, 67, n): the
QPs cycle through the widths 10, 1 and 0.1, from few fixed variables to all of
them; status OK throughout); the backward is fed the GPU's own x and active and
seeded normal cotangents gx and glam, and compared with tests/dual_oracle.py on
the explicit A = [I; -I] (gub = gb[:n], glb = -gb[n:]).  Bars are the
project's (tests/bwd_harness.py): every gradient array within X_TOL = 1e-6 of
the oracle, max|delta| / (1 + max|ref|) per QP, and the certificate of the
outputs on the explicit rows <= KKT_TOL = 1e-9.  The summed gH of one H is held
to shared_cases.sum_bound, (B + 4) 2^-53 sum|products|, against the math.fsum of
the per-QP gH, as in tests/test_gpu_box_shared_backward.py.

Every call goes through the C-ABI (tests/dual_paths_harness.py) into buffers of
the test's own, filled with 0xA5 and fenced by guard words.  The batch of 67
leaves the four-per-wave kernel a ragged last wave.
"""
import itertools

import numpy as np
import pytest

import box_bwd_oracle as BO
import box_dual_oracle as BD
import box_shared_harness as BH
import bwd_cases as BC
import dual_oracle as DO
import dual_paths_harness as DP
import shared_cases as SC
from box_bwd_harness import backward as _plain
from box_bwd_oracle import NAMES
from bwd_harness import KKT_TOL, X_TOL, dev as _dev, rel as _rel

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

OK, MAX_ITER, NOT_SPD, NUMERICAL = 0, 1, 2, 4
B = 67
SEED = 11
SHARED_H = 1
SHAPES = [1, 5, 16, 17, 20, 32]


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    return q


_CASES = {}


def _case(qpb, n):
    """One shape's inputs, its forward on the GPU, the two cotangents and the
    oracle's gradients on the explicit rows: computed once, shared, never modified."""
    if n not in _CASES:
        H, f, lb, ub, _ = BO.cycled(SEED, B, n)
        sol = qpb.solve_box(_dev(H), _dev(f), _dev(lb), _dev(ub))
        torch.cuda.synchronize()
        x, lam, act, st = (t.cpu().numpy() for t in (sol.x, sol.lam, sol.active, sol.status))
        assert (st == OK).all(), st
        mask = qpb.active_mask_to_bool(act, 2 * n)
        rng = np.random.default_rng([SEED, n, 22])
        g, gl = rng.standard_normal((B, n)), rng.standard_normal((B, 2 * n))
        A, _ = BO.dense(lb, ub)
        dm = BO.dense_mask(mask)
        ref = {k: [] for k in NAMES}
        for i in range(B):
            gH, gf, _, gb = DO.backward(H[i], x[i], lam[i], A[i], dm[i], g[i], gl[i])
            for k, v in zip(NAMES, (gH, gf, -gb[n:], gb[:n])):
                ref[k].append(v)
        _CASES[n] = dict(H=H, lb=lb, ub=ub, x=x, lam=lam, act=act, st=st, mask=mask, dm=dm, A=A, g=g, gl=gl,
                         ref={k: np.array(v) for k, v in ref.items()})
    return _CASES[n]


def _run(qpb, c, **kw):
    return DP.box_dual(qpb, kw.pop("shared", 0), kw.pop("H", c["H"]), c["x"], kw.pop("act", c["act"]),
                       kw.pop("st", c["st"]), kw.pop("g", c["g"]), kw.pop("gl", c["gl"]), **kw)


def _prescribed(mask, gl):
    return np.array([BD.prescribed(mask[i], gl[i]) for i in range(len(mask))])


def _certificates(c, out, s=slice(None)):
    gb = BO.to_gb(out["ub"], out["lb"])
    idx = np.arange(B)[s]
    return np.array([DO.certificate(c["H"][i], c["A"][i], c["dm"][i], c["g"][i], c["gl"][i], out["f"][j], gb[j])
                     for j, i in enumerate(idx)])


def _bits_clear_are_zero(out, mask):
    n = mask.shape[1] // 2
    return (out["ub"][~mask[:, :n]] == 0.0).all() and (out["lb"][~mask[:, n:]] == 0.0).all()


# ------------------------------------------------------- parity, certificate, exact dx_S, symmetry
@pytest.mark.parametrize("n", SHAPES)
def test_parity_and_certificate(qpb, n):
    c = _case(qpb, n)
    out = _run(qpb, c)
    assert set(out) == set(NAMES)
    errs = {k: float(_rel(out[k], c["ref"][k]).max()) for k in NAMES}
    cert = _certificates(c, out)
    fixed = c["mask"][:, :n] | c["mask"][:, n:]
    count = fixed.sum(axis=1)
    print(f"n={n}: fixed variables {count.min()}..{count.max()} errors {errs} "
          f"certificate stat {cert[:, 0].max():.2e} prim {cert[:, 1].max():.2e}")
    # the batch reaches from few fixed variables to all of them
    assert count.max() == n and count.min() <= n // 2
    for k in NAMES:
        assert np.isfinite(out[k]).all(), k
        assert errs[k] <= X_TOL, (k, errs[k])
    assert cert.max() <= KKT_TOL, cert.max(axis=0)
    # dx is -glam or +glam on the fixed variables, exactly
    assert np.array_equal(out["f"][fixed], _prescribed(c["mask"], c["gl"])[fixed])
    assert np.array_equal(out["H"], out["H"].transpose(0, 2, 1))
    assert _bits_clear_are_zero(out, c["mask"])
    # the cotangent on lam is not a no-op
    assert not np.array_equal(out["f"], _run(qpb, c, gl=None)["f"])
    # the Python call returns the same bits
    sol = qpb.Solution(_dev(c["x"]), None, _dev(c["act"]), _dev(c["st"]), None)
    got = qpb.solve_box_backward_dual(_dev(c["H"]), sol, _dev(c["g"]), _dev(c["gl"]))
    torch.cuda.synchronize()
    DP.same({k: t.cpu().numpy() for k, t in zip(NAMES, got)}, out, "python")


# ------------------------------------------------------- agreement with qpb_solve_backward_dual
@pytest.mark.parametrize("n", SHAPES)
def test_agrees_with_the_general_dual_backward_on_the_explicit_rows(qpb, n):
    """The same QPs through qpb_solve_backward_dual with A = [I; -I], the box
    solve's lam and the same glam: within X_TOL (not bitwise: that kernel
    orthogonalises the unit rows, this one eliminates them)."""
    c = _case(qpb, n)
    out = _run(qpb, c)
    gen = DP.dual(qpb, 0, c["H"], c["A"], c["x"], c["lam"], c["act"], c["st"], c["g"], c["gl"], need=("H", "f", "b"))
    errs = {"H": _rel(out["H"], gen["H"]).max(), "f": _rel(out["f"], gen["f"]).max(),
            "ub": _rel(out["ub"], gen["b"][:, :n]).max(), "lb": _rel(out["lb"], -gen["b"][:, n:]).max()}
    print(f"n={n}: against qpb_solve_backward_dual {errs}")
    assert max(errs.values()) <= X_TOL, errs


# ------------------------------------------------------- glam NULL is the two existing calls
@pytest.mark.parametrize("n", SHAPES)
def test_null_glam_is_the_box_backward_bit_for_bit(qpb, n):
    c = _case(qpb, n)
    DP.same(_run(qpb, c, gl=None), _plain(qpb, c["H"], c["x"], c["act"], c["st"], c["g"]), "batched H")
    H0 = np.ascontiguousarray(c["H"][0])
    DP.same(_run(qpb, c, shared=SHARED_H, H=H0, gl=None), BH.backward(qpb, H0, c["x"], c["act"], c["st"], c["g"]),
            "one H")
    sol = qpb.Solution(_dev(c["x"]), None, _dev(c["act"]), _dev(c["st"]), None)
    got = qpb.solve_box_backward_dual(_dev(c["H"]), sol, _dev(c["g"]), None)
    torch.cuda.synchronize()
    DP.same({k: t.cpu().numpy() for k, t in zip(NAMES, got)}, _plain(qpb, c["H"], c["x"], c["act"], c["st"], c["g"]),
            "python, glam None")


# ------------------------------------------------------- one H for the batch
@pytest.mark.parametrize("n", SHAPES)
def test_shared_h(qpb, n):
    c = _case(qpb, n)
    H0 = np.ascontiguousarray(c["H"][0])
    ref = _run(qpb, c, H=SC.expand(H0, B))
    got = _run(qpb, c, shared=SHARED_H, H=H0)
    assert got.keys() == ref.keys() and got["H"].shape == (n, n)
    for k in ("f", "lb", "ub"):
        assert DP.bits(got[k], ref[k]), (k, "per-QP output differs")
    none = np.zeros((B, 0))
    bound = SC.sum_bound(c["x"], ref["f"], none, none, np.zeros((B, 0), bool), np.ones(B, bool))[0]
    delta = np.abs(got["H"] - SC.fsum0(ref["H"]))
    assert np.isfinite(got["H"]).all() and (delta <= bound).all(), float((delta - bound).max())
    with np.errstate(invalid="ignore", divide="ignore"):
        print(f"n={n}: worst |delta| / bound of the summed gH {float(np.where(bound > 0, delta / bound, 0.0).max()):.3g}")
    assert DP.bits(got["H"], np.ascontiguousarray(got["H"].T)), "gH is not symmetric bit for bit"
    # every need subset of the shared form, the same call twice and on a side stream: the same bits
    for need in (("H",), ("f",), ("H", "ub"), ("lb", "ub")):
        DP.same(_run(qpb, c, shared=SHARED_H, H=H0, need=need), {k: got[k] for k in need}, need)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    DP.same(_run(qpb, c, shared=SHARED_H, H=H0, stream=side), got, "side stream")
    qpb.release_stream_workspace(side)
    # a poisoned QP contributes exactly 0 to the sum
    st, x = c["st"].copy(), c["x"].copy()
    st[::7], x[::7] = MAX_ITER, np.nan
    gl = np.where((st != OK)[:, None], np.nan, c["gl"])
    bad = DP.box_dual(qpb, SHARED_H, H0, x, c["act"], st, c["g"], gl)
    keep = DP.box_dual(qpb, 0, SC.expand(H0, B), x, c["act"], st, c["g"], gl)
    for k in ("f", "lb", "ub"):
        assert DP.bits(bad[k], keep[k]) and not bad[k][::7].any(), k
    ok = st == OK
    bound = SC.sum_bound(x, keep["f"], none, none, np.zeros((B, 0), bool), ok)[0]
    assert np.isfinite(bad["H"]).all() and (np.abs(bad["H"] - SC.fsum0(keep["H"][ok])) <= bound).all()
    # the Python call with a 2-D H
    sol = qpb.Solution(_dev(c["x"]), None, _dev(c["act"]), _dev(c["st"]), None)
    out = qpb.solve_box_backward_dual(_dev(H0), sol, _dev(c["g"]), _dev(c["gl"]))
    torch.cuda.synchronize()
    DP.same({k: t.cpu().numpy() for k, t in zip(NAMES, out)}, got, "python, 2-D H")


# ------------------------------------------------------- hand-made masks
HAND = 8


def _hand(qpb, n):
    c = _case(qpb, n)
    s = slice(0, HAND)
    return c, c["H"][s], c["x"][s], c["st"][s], c["g"][s], c["mask"][s], c["gl"][s]


def _oracle(H, x, mask, g, gl):
    return BD.backward_batch(H, x, mask, g, gl)


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
    gl[rows, n + var] = np.nan
    out = DP.box_dual(qpb, 0, H, x, BC.words(mask), st, g, gl)
    ref = _oracle(H, x, mask, g, gl)
    for k in NAMES:
        assert np.isfinite(out[k]).all(), k
        assert _rel(out[k], ref[k]).max() <= X_TOL, k
    assert (out["lb"][rows, var] == 0.0).all()
    assert np.array_equal(out["f"][rows, var], -gl[rows, var])
    r = g + np.einsum("bij,bj->bi", H, out["f"])
    assert np.abs(out["ub"][rows, var] - r[rows, var]).max() <= X_TOL * (1 + np.abs(r).max())
    assert _bits_clear_are_zero(out, mask)


@pytest.mark.parametrize("n", SHAPES)
def test_all_bits_set(qpb, n):
    """Every variable fixed at its upper bound (both bits set): gf = d = -glam[:n],
    gH from it, r = gx + H d on the upper bounds, nothing on the lower ones."""
    c, H, x, st, g, _, gl = _hand(qpb, n)
    gl = gl.copy()
    gl[:, n:] = np.nan
    out = DP.box_dual(qpb, 0, H, x, BC.words(np.ones((HAND, 2 * n), bool)), st, g, gl)
    d = -gl[:, :n]
    assert np.array_equal(out["f"], d) and (out["lb"] == 0.0).all()
    gH = 0.5 * (np.einsum("bi,bj->bij", d, x) + np.einsum("bi,bj->bij", x, d))
    assert _rel(out["H"], gH).max() <= 4 * 2.0 ** -53  # two products and a sum, each rounded once
    assert np.array_equal(out["H"], out["H"].transpose(0, 2, 1))
    r = g + np.einsum("bij,bj->bi", H, d)
    assert _rel(out["ub"], r).max() <= X_TOL
    # all at their lower bounds: d = +glam[n:]
    low = np.zeros((HAND, 2 * n), bool)
    low[:, n:] = True
    gl2 = c["gl"][:HAND].copy()
    gl2[:, :n] = np.nan
    out = DP.box_dual(qpb, 0, H, x, BC.words(low), st, g, gl2)
    assert np.array_equal(out["f"], gl2[:, n:]) and (out["ub"] == 0.0).all()
    assert _rel(out["lb"], g + np.einsum("bij,bj->bi", H, gl2[:, n:])).max() <= X_TOL


@pytest.mark.parametrize("n", SHAPES)
def test_no_bit_set(qpb, n):
    """None fixed: glam -- all NaN -- is wholly ignored, the old outputs bit for bit."""
    c, H, x, st, g, _, _ = _hand(qpb, n)
    act = BC.words(np.zeros((HAND, 2 * n), bool))
    out = DP.box_dual(qpb, 0, H, x, act, st, g, np.full((HAND, 2 * n), np.nan))
    DP.same(out, _plain(qpb, H, x, act, st, g), "no bit set")
    assert np.isfinite(out["f"]).all() and (out["lb"] == 0.0).all() and (out["ub"] == 0.0).all()


@pytest.mark.parametrize("n", [1, 5, 17, 20])  # (n = 16 and 32 fill their words: no position >= 2n)
def test_bits_past_2n_are_ignored(qpb, n):
    c, H, x, st, g, mask, gl = _hand(qpb, n)
    act = BC.words(mask)
    gl = np.where(mask, gl, np.nan)  # NaN at every clear bit
    clean = DP.box_dual(qpb, 0, H, x, act, st, g, c["gl"][:HAND])
    last = act.view(np.uint32).copy()
    spare = np.uint32((0xFFFFFFFF << ((2 * n) % 32)) & 0xFFFFFFFF)
    last[:, -1] |= spare & np.uint32(0xDEADBEEF | (1 << 31) | (1 << ((2 * n) % 32)))
    assert (last[:, -1] != act.view(np.uint32)[:, -1]).all()
    DP.same(DP.box_dual(qpb, 0, H, x, last.view(np.int32), st, g, gl), clean, "bits past 2n")
    DP.same(clean, {k: v[:HAND] for k, v in _run(qpb, c).items()}, "the first QPs of the batch")


# ------------------------------------------------------- poisoned QPs, NULL outputs, NULL status
@pytest.mark.parametrize("n", SHAPES)
def test_poisoned_qps_get_zeros(qpb, n):
    c = _case(qpb, n)
    bad = np.zeros(B, bool)
    bad[::7] = True
    x, st = c["x"].copy(), c["st"].copy()
    st[bad] = np.resize([MAX_ITER, NOT_SPD, NUMERICAL], bad.sum())
    x[bad] = np.nan
    ignored = ~c["dm"] | bad[:, None]
    poisoned = np.where(ignored, np.nan, c["gl"])
    got = DP.box_dual(qpb, 0, c["H"], x, c["act"], st, c["g"], poisoned)
    full = _run(qpb, c)
    for k in NAMES:
        assert np.isfinite(got[k]).all(), k
        assert (got[k][bad] == 0.0).all(), k
        assert DP.bits(got[k][~bad], full[k][~bad]), k


@pytest.mark.parametrize("n", SHAPES)
def test_every_need_subset_and_null_status(qpb, n):
    c = _case(qpb, n)
    full = _run(qpb, c)
    for r in range(1, 4):
        for need in itertools.combinations(NAMES, r):
            got = _run(qpb, c, need=need)
            assert set(got) == set(need)
            DP.same(got, {k: full[k] for k in need}, need)
    DP.same(_run(qpb, c, st=None), full, "status NULL")
    sol = qpb.Solution(_dev(c["x"]), None, _dev(c["act"]), None, None)
    gH, gf, glb, gub = qpb.solve_box_backward_dual(_dev(c["H"]), sol, _dev(c["g"]), _dev(c["gl"]), need=("f", "ub"))
    torch.cuda.synchronize()
    assert gH is None and glb is None
    DP.same({"f": gf.cpu().numpy(), "ub": gub.cpu().numpy()}, {"f": full["f"], "ub": full["ub"]}, "python need")


# ------------------------------------------------------- independence, streams, the host call
@pytest.mark.parametrize("n", SHAPES)
def test_a_qp_depends_on_its_own_inputs_only(qpb, n):
    """A QP's bits at two batch positions and sizes, and with its neighbours poisoned."""
    c = _case(qpb, n)
    full = _run(qpb, c)
    k = 5
    one = slice(k, k + 1)
    alone = DP.box_dual(qpb, 0, c["H"][one], c["x"][one], c["act"][one], c["st"][one], c["g"][one], c["gl"][one])
    DP.same(alone, {j: v[one] for j, v in full.items()}, "alone")
    perm = np.random.default_rng(SEED).permutation(B)[:31]
    moved = DP.box_dual(qpb, 0, c["H"][perm], c["x"][perm], c["act"][perm], c["st"][perm], c["g"][perm], c["gl"][perm])
    DP.same(moved, {j: v[perm] for j, v in full.items()}, "permuted, 31 QPs")
    arrays = {j: c[j].copy() for j in ("H", "x", "g", "gl")}
    others = np.arange(B) != k
    for v in arrays.values():
        v[others] = np.nan
    poisoned = DP.box_dual(qpb, 0, arrays["H"], arrays["x"], c["act"], c["st"], arrays["g"], arrays["gl"])
    DP.same({j: v[one] for j, v in poisoned.items()}, alone, "neighbours poisoned")


@pytest.mark.parametrize("n", SHAPES)
def test_side_stream_and_host_call(qpb, n):
    c = _case(qpb, n)
    full = _run(qpb, c)
    torch.cuda.synchronize()
    DP.same(_run(qpb, c, stream=torch.cuda.Stream()), full, "side stream")
    hs = qpb.Solution(c["x"], None, c["act"], c["st"], None)
    DP.same(dict(zip(NAMES, qpb.solve_box_backward_dual_host(c["H"], hs, c["g"], c["gl"]))), full, "host")
    H0 = np.ascontiguousarray(c["H"][0])
    shared = _run(qpb, c, shared=SHARED_H, H=H0)
    DP.same(dict(zip(NAMES, qpb.solve_box_backward_dual_host(H0, hs, c["g"], c["gl"]))), shared, "host, one H")
    gH, gf, glb, gub = qpb.solve_box_backward_dual_host(c["H"], hs, c["g"], c["gl"], need=("lb",))
    assert gH is None and gf is None and gub is None and DP.bits(glb, full["lb"])


def test_above_the_wave_class_is_unsupported(qpb):
    n, Bq = 33, 2
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")  # noqa: E731
    act = torch.zeros((Bq, (2 * n + 31) // 32), dtype=torch.int32, device="cuda")
    sol = qpb.Solution(z(Bq, n), None, act, None, None)
    with pytest.raises(qpb.QPBError) as e:
        qpb.solve_box_backward_dual(z(Bq, n, n), sol, z(Bq, n), z(Bq, 2 * n))
    assert e.value.code == qpb.ERR_UNSUPPORTED and "n<=32" in str(e.value)


# ------------------------------------------------------- ill-conditioned H
def _cond_case(n):
    """tests/test_gpu_box_backward.py's: H of cond 1e3, 1e6, 1e10
    (bwd_cases.conditioned_inputs, its H only), each with about a third of the
    variables fixed and with all but one, at the upper or the lower bound at
    random; and a normal glam."""
    Hs, *_, ps, _ = BC.conditioned_inputs(n, 2 * n)
    rs = np.random.default_rng([131, n])
    H, mask, p, kind = [], [], [], []
    for Hq, pq in zip(Hs, ps):
        for kd in ("third", "all_but_one"):
            fixed = rs.permutation(n)[:n // 3] if kd == "third" else np.delete(np.arange(n), rs.integers(n))
            mk = np.zeros(2 * n, bool)
            mk[fixed + n * (rs.random(len(fixed)) < 0.5)] = True
            H.append(Hq)
            mask.append(mk)
            p.append(pq)
            kind.append(kd)
    Bq = len(H)
    return (np.array(H), rs.standard_normal((Bq, n)), np.array(mask), rs.standard_normal((Bq, n)),
            rs.standard_normal((Bq, 2 * n)), np.array(p), np.array(kind))


@pytest.mark.parametrize("n", [16, 32])
def test_ill_conditioned_h(qpb, n):
    """cond(H) = 1e3, 1e6, 1e10.  The bar on dual_oracle.certificate (on the
    explicit A) is, as in tests/test_gpu_box_backward.py, per QP and residual
    100 x the certificate of the numpy closed form's own outputs on the same
    inputs, floored at bwd_cases.COND_FLOOR: the kernel eliminates in another
    order in the same precision.  The primal residual is exactly 0: dx is the
    prescribed value on every fixed variable."""
    H, x, mask, g, gl, p, kind = _cond_case(n)
    assert len(H) == 30 and set(p) == set(BC.COND_EXPONENTS)
    A = BO.dense(np.zeros((1, n)), np.zeros((1, n)))[0][0]

    def certs(out):
        gb = BO.to_gb(out["ub"], out["lb"])
        return np.array([DO.certificate(H[i], A, mask[i], g[i], gl[i], out["f"][i], gb[i]) for i in range(len(H))])

    ref = BD.backward_batch(H, x, mask, g, gl)
    oracle = certs(ref)
    out = DP.box_dual(qpb, 0, H, x, BC.words(mask), None, g, gl)
    cert = certs(out)
    for e in BC.COND_EXPONENTS:
        for kd in ("third", "all_but_one"):
            s = (p == e) & (kind == kd)
            print(f"n={n} cond 1e{e} {kd}: oracle stat {oracle[s, 0].max():.2e} prim {oracle[s, 1].max():.2e} | "
                  f"GPU stat {cert[s, 0].max():.2e} prim {cert[s, 1].max():.2e} | "
                  f"gf against the oracle {_rel(out['f'][s], ref['f'][s]).max():.2e}")
    for k in NAMES:
        assert np.isfinite(out[k]).all(), k
    bar = np.maximum(BC.COND_FLOOR, 100.0 * oracle)
    assert (cert <= bar).all(), (cert / bar).max()
    fixed = mask[:, :n] | mask[:, n:]
    assert np.array_equal(out["f"][fixed], _prescribed(mask, gl)[fixed]) and _bits_clear_are_zero(out, mask)
    assert (cert[:, 1] == 0.0).all()
    assert np.array_equal(out["H"], out["H"].transpose(0, 2, 1))
