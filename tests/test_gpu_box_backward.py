"""qpb_solve_box_backward on the GPU: the gradients of a box solve, in both
kernels of qpb_kkt_bwd_box.hip (n <= 16: four QPs per wavefront, with its
n < 16 and n == 16 load / store paths; 16 < n <= 32: one QP per wavefront, the
mask straddling its two words at n = 17 and 20 and filling them at n = 32).

The forward is qpb.solve_box on the GPU (box_bwd_oracle.cycled(11, 67, n): the
QPs cycle through the widths 10, 1 and 0.1, so the neighbours in a wavefront
have different masks, from no fixed variable to all of them; status OK
throughout); the backward is fed the GPU's own x and active, and compared with
tests/kkt_oracle.py on the explicit A = [I; -I] (gub = gb[:n], glb = -gb[n:]).
Bars are test_gpu_backward.py's: every gradient array within X_TOL = 1e-6 of
the oracle, max|delta| / (1 + max|ref|) per QP, and the certificate of the
outputs on the explicit A <= KKT_TOL = 1e-9.

Every call goes through the C-ABI (tests/box_bwd_harness.py) into buffers of
the test's own, filled with 0xA5 and fenced by guard words: each test also
checks that every element was written and nothing outside.  "Bitwise" compares
two launches on the same QP.  The batch of 67 leaves the four-per-wave kernel
a ragged last wave.
"""
import numpy as np
import pytest

import box_bwd_oracle as BO
import bwd_cases as BC
from box_bwd_harness import backward as _backward
from box_bwd_oracle import NAMES
from bwd_harness import KKT_TOL, X_TOL
from bwd_harness import backward as _dense_backward, dev as _dev, rel as _rel, same as _same

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

OK, MAX_ITER, NOT_SPD = 0, 1, 2
B = 67
SEED = 11

DENSE_SHAPES = [1, 5, 16]
WAVE_SHAPES = [17, 20, 32]
# one shape per load / store path: n < 16, n == 16, the wave kernel
PATH_SHAPES = [5, 16, 20]


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    return q


def _forward(qpb, H, f, lb, ub, **kw):
    """solve_box on the GPU; numpy (x, lam, active words, status)."""
    sol = qpb.solve_box(_dev(H), _dev(f), _dev(lb), _dev(ub), **kw)
    torch.cuda.synchronize()
    return sol.x.cpu().numpy(), sol.lam.cpu().numpy(), sol.active.cpu().numpy(), sol.status.cpu().numpy()


_CASES = {}


def _case(qpb, n):
    """One shape's inputs, its forward on the GPU, the cotangent and the
    oracle's gradients: computed once, shared, never modified."""
    if n not in _CASES:
        H, f, lb, ub, width = BO.cycled(SEED, B, n)
        x, lam, act, st = _forward(qpb, H, f, lb, ub)
        assert (st == OK).all(), st
        mask = qpb.active_mask_to_bool(act, 2 * n)
        g = np.random.default_rng([SEED, n]).standard_normal((B, n))
        ref = BO.dense_form(H, x, mask, g)
        _CASES[n] = dict(H=H, f=f, lb=lb, ub=ub, x=x, lam=lam, act=act, st=st, mask=mask, g=g, ref=ref, width=width)
    return _CASES[n]


def _run(qpb, c, **kw):
    return _backward(qpb, c["H"], c["x"], c["act"], kw.pop("st", c["st"]), c["g"], **kw)


def _bits_clear_are_zero(out, mask):
    n = mask.shape[1] // 2
    return (out["ub"][~mask[:, :n]] == 0.0).all() and (out["lb"][~mask[:, n:]] == 0.0).all()


# ------------------------------------------------------- parity, certificate, symmetry
@pytest.mark.parametrize("n", DENSE_SHAPES + WAVE_SHAPES)
def test_parity_and_certificate(qpb, n):
    c = _case(qpb, n)
    out = _run(qpb, c)
    assert set(out) == set(NAMES)
    errs = {k: float(_rel(out[k], c["ref"][k]).max()) for k in NAMES}
    cert = BO.certificates(c["H"], c["mask"], c["g"], out)
    fixed = (c["mask"][:, :n] | c["mask"][:, n:]).sum(axis=1)
    print(f"n={n}: fixed variables {fixed.min()}..{fixed.max()} errors {errs} "
          f"certificate stat {cert[:, 0].max():.2e} prim {cert[:, 1].max():.2e}")
    # the batch reaches from no fixed variable (n <= 5) or few to all of them
    assert fixed.max() == n and fixed.min() <= n // 2
    for k in NAMES:
        assert np.isfinite(out[k]).all(), k
        assert errs[k] <= X_TOL, (k, errs[k])
    assert cert.max() <= KKT_TOL, cert.max(axis=0)
    assert np.array_equal(out["H"], out["H"].transpose(0, 2, 1))
    assert _bits_clear_are_zero(out, c["mask"])
    # dx is exactly zero on the fixed variables
    assert (out["f"][c["mask"][:, :n] | c["mask"][:, n:]] == 0.0).all()
    # the Python call returns the same bits
    sol = qpb.Solution(_dev(c["x"]), None, _dev(c["act"]), _dev(c["st"]), None)
    got = qpb.solve_box_backward(_dev(c["H"]), sol, _dev(c["g"]))
    torch.cuda.synchronize()
    assert _same(out, {k: t.cpu().numpy() for k, t in zip(NAMES, got)})


# ------------------------------------------------------- agreement with qpb_solve_backward
@pytest.mark.parametrize("n", DENSE_SHAPES + WAVE_SHAPES)
def test_agrees_with_the_general_backward_on_the_explicit_rows(qpb, n):
    """The same QPs through qpb_solve_backward with A = [I; -I] and the box
    solve's lam: the same gradients within X_TOL (not bitwise: that kernel
    orthogonalises the unit rows, this one eliminates them)."""
    c = _case(qpb, n)
    out = _run(qpb, c)
    A, _ = BO.dense(c["lb"], c["ub"])
    gen = _dense_backward(qpb, c["H"], A, c["x"], c["lam"], c["act"], c["st"], c["g"], need=("H", "f", "b"))
    errs = {"H": _rel(out["H"], gen["H"]).max(), "f": _rel(out["f"], gen["f"]).max(),
            "ub": _rel(out["ub"], gen["b"][:, :n]).max(), "lb": _rel(out["lb"], -gen["b"][:, n:]).max()}
    print(f"n={n}: against qpb_solve_backward {errs}")
    assert max(errs.values()) <= X_TOL, errs


# ------------------------------------------------------- everything written, zeros where due
@pytest.mark.parametrize("n", PATH_SHAPES)
@pytest.mark.parametrize("how", ["not_spd", "max_iter"])
def test_non_ok_qps_get_zeros(qpb, n, how):
    c = _case(qpb, n)
    H = c["H"].copy()
    kw = {}
    if how == "not_spd":
        H[3] = -np.eye(n)
    else:
        kw["max_iter"] = 1
    x, lam, act, st = _forward(qpb, H, c["f"], c["lb"], c["ub"], **kw)
    assert ((st == NOT_SPD) == (np.arange(B) == 3)).all() if how == "not_spd" else (st == MAX_ITER).any(), st
    out = _backward(qpb, H, x, act, st, c["g"])  # (guards and written-ness checked inside)
    bad = st != OK
    mask = qpb.active_mask_to_bool(act, 2 * n)
    for k in NAMES:
        assert (out[k][bad] == 0.0).all(), k
        assert np.isfinite(out[k]).all(), k
    good = ~bad
    assert _bits_clear_are_zero({k: v[good] for k, v in out.items()}, mask[good])
    if how == "not_spd":  # the others are the unchanged QPs of the shared case
        ref = {k: v[good] for k, v in _run(qpb, c).items()}
        assert _same({k: v[good] for k, v in out.items()}, ref)


# ------------------------------------------------------- NULL outputs, NULL status
@pytest.mark.parametrize("n", PATH_SHAPES)
def test_null_outputs_and_null_status(qpb, n):
    c = _case(qpb, n)
    full = _run(qpb, c)
    for k in NAMES:
        one = _run(qpb, c, need=(k,))
        assert _same(one, {k: full[k]}), k
        three = tuple(j for j in NAMES if j != k)
        assert _same(_run(qpb, c, need=three), {j: full[j] for j in three}), three
    assert _same(_run(qpb, c, st=None), full)
    # the Python call: what is left out of `need` comes back as None
    sol = qpb.Solution(_dev(c["x"]), None, _dev(c["act"]), None, None)
    gH, gf, glb, gub = qpb.solve_box_backward(_dev(c["H"]), sol, _dev(c["g"]), need=("f", "ub"))
    torch.cuda.synchronize()
    assert gH is None and glb is None
    assert _same({"f": gf.cpu().numpy(), "ub": gub.cpu().numpy()}, {"f": full["f"], "ub": full["ub"]})


# ------------------------------------------------------- independence
@pytest.mark.parametrize("n", PATH_SHAPES)
def test_a_qp_depends_on_its_own_inputs_only(qpb, n):
    c = _case(qpb, n)
    full = _run(qpb, c)
    k = 5
    one = slice(k, k + 1)
    alone = _backward(qpb, c["H"][one], c["x"][one], c["act"][one], c["st"][one], c["g"][one])
    assert _same(alone, {j: v[one] for j, v in full.items()})
    arrays = {j: c[j].copy() for j in ("H", "x", "g")}
    others = np.arange(B) != k
    for v in arrays.values():
        v[others] = np.nan
    poisoned = _backward(qpb, arrays["H"], arrays["x"], c["act"], c["st"], arrays["g"])
    assert _same({j: v[one] for j, v in poisoned.items()}, alone)


# ------------------------------------------------------- streams
@pytest.mark.parametrize("n", PATH_SHAPES)
def test_non_default_stream_gives_the_same_bits(qpb, n):
    c = _case(qpb, n)
    full = _run(qpb, c)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert _same(_run(qpb, c, stream=s), full)


# ------------------------------------------------------- the host-pointer call
@pytest.mark.parametrize("n", PATH_SHAPES)
def test_host_call_gives_the_same_bits(qpb, n):
    c = _case(qpb, n)
    full = _run(qpb, c)
    got = qpb.solve_box_backward_host(c["H"], qpb.Solution(c["x"], None, c["act"], c["st"], None), c["g"])
    assert _same(full, dict(zip(NAMES, got)))
    sol = qpb.Solution(c["x"], None, c["act"], None, None)
    gH, gf, glb, gub = qpb.solve_box_backward_host(c["H"], sol, c["g"], need=("lb",))
    assert gH is None and gf is None and gub is None
    assert _same({"lb": glb}, {"lb": full["lb"]})


# ------------------------------------------------------- the size limit
def test_above_the_wave_class_is_unsupported(qpb):
    n, Bq = 33, 2
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")  # noqa: E731
    act = torch.zeros((Bq, (2 * n + 31) // 32), dtype=torch.int32, device="cuda")
    sol = qpb.Solution(z(Bq, n), None, act, None, None)
    with pytest.raises(qpb.QPBError) as e:
        qpb.solve_box_backward(z(Bq, n, n), sol, z(Bq, n))
    assert e.value.code == qpb.ERR_UNSUPPORTED and "n<=32" in str(e.value)


# ------------------------------------------------------- hand-made masks
HAND = 8


def _hand(qpb, n):
    c = _case(qpb, n)
    s = slice(0, HAND)
    return c, c["H"][s], c["x"][s], c["st"][s], c["g"][s], c["mask"][s]


@pytest.mark.parametrize("n", PATH_SHAPES)
def test_both_bits_of_a_variable_set(qpb, n):
    """The upper bound counts and the lower bound gets 0; everything else is
    the system with that one (upper) row."""
    c, H, x, st, g, mask = _hand(qpb, n)
    mask = mask.copy()
    var = np.arange(HAND) * 3 % n
    mask[np.arange(HAND), var] = True
    mask[np.arange(HAND), n + var] = True
    out = _backward(qpb, H, x, BC.words(mask), st, g)
    ref = BO.dense_form(H, x, mask, g)  # (dense_mask drops the lower bit)
    for k in NAMES:
        assert np.isfinite(out[k]).all(), k
        assert _rel(out[k], ref[k]).max() <= X_TOL, k
    assert (out["lb"][np.arange(HAND), var] == 0.0).all()
    # gub = r = gx + H dx on that variable
    r = g + np.einsum("bij,bj->bi", H, out["f"])
    assert np.abs(out["ub"][np.arange(HAND), var] - r[np.arange(HAND), var]).max() <= X_TOL * (1 + np.abs(r).max())
    assert _bits_clear_are_zero(out, mask)


@pytest.mark.parametrize("n", PATH_SHAPES)
def test_all_bits_set(qpb, n):
    c, H, x, st, g, _ = _hand(qpb, n)
    out = _backward(qpb, H, x, BC.words(np.ones((HAND, 2 * n), bool)), st, g)
    assert (out["f"] == 0.0).all() and (out["H"] == 0.0).all() and (out["lb"] == 0.0).all()
    assert np.array_equal(out["ub"], g)


@pytest.mark.parametrize("n", PATH_SHAPES)
def test_no_bit_set(qpb, n):
    c, H, x, st, g, _ = _hand(qpb, n)
    out = _backward(qpb, H, x, BC.words(np.zeros((HAND, 2 * n), bool)), st, g)
    dx = -np.linalg.solve(H, g[..., None])[..., 0]
    assert _rel(out["f"], dx).max() <= X_TOL
    gH = 0.5 * (np.einsum("bi,bj->bij", dx, x) + np.einsum("bi,bj->bij", x, dx))
    assert _rel(out["H"], gH).max() <= X_TOL
    assert (out["lb"] == 0.0).all() and (out["ub"] == 0.0).all()


@pytest.mark.parametrize("n", [5, 20])  # (n = 16 fills its word: no position >= 2n)
def test_bits_past_2n_are_ignored(qpb, n):
    c, H, x, st, g, mask = _hand(qpb, n)
    act = BC.words(mask)
    clean = _backward(qpb, H, x, act, st, g)
    last = act.view(np.uint32).copy()
    spare = np.uint32((0xFFFFFFFF << ((2 * n) % 32)) & 0xFFFFFFFF)
    last[:, -1] |= spare & np.uint32(0xDEADBEEF | (1 << 31) | (1 << ((2 * n) % 32)))
    assert (last[:, -1] != act.view(np.uint32)[:, -1]).all()
    assert _same(_backward(qpb, H, x, last.view(np.int32), st, g), clean)
    assert _same(clean, {k: v[:HAND] for k, v in _run(qpb, c).items()})


# ------------------------------------------------------- ill-conditioned H
def _cond_case(n):
    """H of cond 1e3, 1e6, 1e10 (bwd_cases.conditioned_inputs, its H only), each
    under two masks of the test's own: about a third of the variables fixed,
    and all but one; a fixed variable's bound is the upper or the lower one at
    random.  Returns (H, x, mask, g, p, kind)."""
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
    return (np.array(H), rs.standard_normal((Bq, n)), np.array(mask), rs.standard_normal((Bq, n)), np.array(p),
            np.array(kind))


@pytest.mark.parametrize("n", [16, 32])
def test_ill_conditioned_h(qpb, n):
    """cond(H) = 1e3, 1e6, 1e10 with a third of the variables fixed and with
    all but one.  The bar on kkt_oracle.certificate (on the explicit A) is per
    QP and residual 100 x the certificate of the numpy oracle's own outputs on
    the same inputs, floored at bwd_cases.COND_FLOOR = 1.89e-13: the kernel
    eliminates in another order in the same precision.

    Measured on an MI355X (kkt_bwd_box v1.0): the worst stationarity residual,
    numpy oracle | GPU (the primal residual is exactly 0 for both: dx is an
    exact zero on every fixed variable), and gf against the oracle:
      n   cond   a third fixed                 all but one fixed
      16  1e3    4.4e-17 | 5.4e-17  9.1e-15    1.0e-16 | 3.0e-17  1.5e-15
      16  1e6    1.6e-17 | 1.8e-17  3.8e-13    2.8e-17 | 8.3e-17  1.2e-15
      16  1e10   3.3e-17 | 2.3e-17  1.2e-10    3.5e-17 | 1.6e-17  7.0e-16
      32  1e3    2.4e-17 | 5.2e-17  7.3e-15    1.8e-17 | 1.8e-17  8.5e-17
      32  1e6    2.3e-17 | 2.2e-17  7.8e-13    1.2e-16 | 3.0e-17  5.2e-16
      32  1e10   2.4e-17 | 2.3e-17  3.8e-10    1.7e-17 | 5.9e-18  2.6e-15
    Every figure is under the floor: the bar in force is the floor itself.
    """
    H, x, mask, g, p, kind = _cond_case(n)
    assert len(H) == 30 and set(p) == set(BC.COND_EXPONENTS)
    ref = BO.dense_form(H, x, mask, g)
    oracle = BO.certificates(H, mask, g, ref)
    out = _backward(qpb, H, x, BC.words(mask), None, g)
    cert = BO.certificates(H, mask, g, out)
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
    assert (out["f"][fixed] == 0.0).all() and _bits_clear_are_zero(out, mask)
    assert np.array_equal(out["H"], out["H"].transpose(0, 2, 1))
