"""CPU tests of the oracle for qpb_solve_box_backward (tests/box_bwd_oracle.py):
the reduced formulas of a box (one solve on the free variables, r = g + H dx
on the active bounds) agree with tests/kkt_oracle.py on the explicit
A = [I; -I], and the families the GPU tests use cover the ground they are
chosen for.  The forward is oracle.active_set_solve on the dense form.

Measured here (seed 11, 67 QPs): the worst disagreement is 4.9e-14 in
bwd_harness.rel's measure at cond(H) ~ 1e3 (the bar is 1e-11, a hundred times
the 1e-13 that two fp64 eliminations of such an H may differ by); the active
bounds per QP at widths
10 / 1 / 0.1 are 1-8 / 8-16 / 12-16 at n = 16 and 4-15 / 19-30 / 29-32 at
n = 32.
"""
import numpy as np
import pytest

import box_bwd_oracle as BO
import bwd_cases as BC
import kkt_oracle as KO
from bwd_harness import rel

SEED = 11
B = 67
SIZES = [1, 5, 16, 20, 32]
AGREE_TOL = 1e-11

_SOLVED = {}


def _solved(n, width):
    """One (n, width)'s family, its forward on the CPU and a cotangent: computed once, never modified."""
    key = (n, width)
    if key not in _SOLVED:
        H, f, lb, ub = BO.family(SEED, B, n, width)
        x, lam, mask = BO.solve(H, f, lb, ub)
        g = np.random.default_rng([SEED, n, int(round(width * 10))]).standard_normal((B, n))
        _SOLVED[key] = dict(H=H, f=f, lb=lb, ub=ub, x=x, lam=lam, mask=mask, g=g)
    return _SOLVED[key]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("width", BO.WIDTHS)
def test_reduced_formulas_agree_with_the_dense_kkt_system(n, width):
    c = _solved(n, width)
    got = BO.backward_batch(c["H"], c["x"], c["mask"], c["g"])
    A, _ = BO.dense(c["lb"], c["ub"])
    worst = 0.0
    for i in range(B):
        # the forward's own lam here: gA is not compared, gH, gf and gb do not depend on it
        gH, gf, _, gb = KO.backward(c["H"][i], c["x"][i], c["lam"][i], A[i], BO.dense_mask(c["mask"][i]), c["g"][i])
        ref = {"H": gH, "f": gf, "ub": gb[:n], "lb": -gb[n:]}
        for k in BO.NAMES:
            worst = max(worst, float(rel(got[k][i][None], ref[k][None])[0]))
    cert = BO.certificates(c["H"], c["mask"], c["g"], got)
    print(f"n={n} width={width}: active {c['mask'].sum(axis=1).min()}..{c['mask'].sum(axis=1).max()} "
          f"worst disagreement {worst:.2e} certificate {cert.max(axis=0)}")
    assert worst <= AGREE_TOL
    assert cert.max() <= 1e-12
    # the gradient of a bound is zero where its bit is clear, and gH is symmetric bit for bit
    assert (got["ub"][~c["mask"][:, :n]] == 0.0).all() and (got["lb"][~c["mask"][:, n:]] == 0.0).all()
    assert np.array_equal(got["H"], got["H"].transpose(0, 2, 1))
    # dense_form is the same reference, batched, without lam
    ref = BO.dense_form(c["H"], c["x"], c["mask"], c["g"])
    assert max(float(rel(got[k], ref[k]).max()) for k in BO.NAMES) <= AGREE_TOL


def test_the_families_cover_the_ground():
    fixed = {(n, w): (lambda m: (m[:, :n] | m[:, n:]).sum(axis=1))(_solved(n, w)["mask"])
             for n in SIZES for w in BO.WIDTHS}
    # no fixed variable at all somewhere at a small size and the widest box
    assert (fixed[(1, 10.0)] == 0).any() or (fixed[(5, 10.0)] == 0).any()
    # every variable fixed somewhere at the narrowest box
    for n in SIZES:
        if n >= 5:
            assert (fixed[(n, 0.1)] == n).any(), n
    # the three widths reach from few active bounds to nearly all
    for n in (16, 32):
        print(n, {w: (int(fixed[(n, w)].min()), int(fixed[(n, w)].max())) for w in BO.WIDTHS})
        assert fixed[(n, 10.0)].max() <= n // 2 and fixed[(n, 0.1)].min() >= 3 * n // 4


@pytest.mark.parametrize("n", SIZES)
def test_the_widest_box_is_safe_for_a_finite_difference(n):
    """At width 10 every active multiplier is >= 0.19 and every inactive slack
    >= 1e-2: a step of 1e-6 along any unit direction keeps the active set."""
    c = _solved(n, 10.0)
    _, b = BO.dense(c["lb"], c["ub"])
    slack = b - np.concatenate([c["x"], -c["x"]], axis=1)
    assert c["lam"][c["mask"]].min() >= 0.19 if c["mask"].any() else True
    assert slack[~c["mask"]].min() >= 1e-2


def test_helpers():
    n = 3
    mask = np.array([[1, 0, 1, 1, 1, 0]], bool)  # variable 0: both bits; 1: lower; 2: upper
    assert BO.dense_mask(mask).tolist() == [[True, False, True, False, True, False]]
    assert BC.words(mask).tolist() == [[0b011101]]
    gub, glb = np.array([[1.0, 0.0, 3.0]]), np.array([[0.0, 2.0, 0.0]])
    assert BO.to_gb(gub, glb).tolist() == [[1.0, 0.0, 3.0, -0.0, -2.0, -0.0]]
    H = np.array([[[2.0, 1.0, 0.0], [1.0, 2.0, 1.0], [0.0, 1.0, 2.0]]])
    g = np.array([[1.0, 2.0, 3.0]])
    x = np.array([[1.0, -1.0, 0.5]])
    out = BO.backward_batch(H, x, np.ones((1, 2 * n), bool), g)  # all fixed: gf = 0, gH = 0, gub = g
    assert (out["f"] == 0).all() and (out["H"] == 0).all() and (out["lb"] == 0).all()
    assert np.array_equal(out["ub"], g)
    out = BO.backward_batch(H, x, np.zeros((1, 2 * n), bool), g)  # none fixed: dx = -H^{-1} g
    assert np.allclose(out["f"][0], -np.linalg.solve(H[0], g[0])) and (out["lb"] == 0).all() and (out["ub"] == 0).all()
    Hc, fc, lbc, ubc, w = BO.cycled(SEED, 7, n)
    assert w.tolist() == [10.0, 1.0, 0.1, 10.0, 1.0, 0.1, 10.0] and (lbc < 0).all() and (ubc > 0).all()
    assert np.array_equal(Hc[1], BO.family(SEED, 7, n, 1.0)[0][1])
