"""CPU tests of the oracle for qpb_solve_box_backward_dual (tests/box_dual_oracle.py).

The closed form (a prescribed dx on the fixed variables, one solve on the free
ones) agrees with tests/dual_oracle.py on the explicit rows of
box_bwd_oracle.dense to 1e-12 in bwd_harness.rel's measure, and its tangent
agrees with central differences of the CPU forward (box_bwd_oracle.solve): step
1e-6 and bar 1e-4 as in tests/test_gpu_tangent.py, on the widest box, where
tests/test_box_bwd_oracle.py shows that such a step keeps the active set (every
active multiplier >= 0.19, every inactive slack >= 1e-2) -- and the test checks
that it did.
"""
import numpy as np
import pytest

import box_bwd_oracle as BO
import box_dual_oracle as BD
import dual_oracle as DO
from bwd_harness import rel

SEED = 11
B = 67
SIZES = [1, 5, 16, 17, 20, 32]
AGREE_TOL = 1e-12
EPS, FD_TOL = 1e-6, 1e-4


@pytest.mark.parametrize("n", SIZES)
def test_closed_form_agrees_with_the_dense_kkt_system(n):
    H, f, lb, ub, _ = BO.cycled(SEED, B, n)
    x, lam, mask = BO.solve(H, f, lb, ub)
    rng = np.random.default_rng([SEED, n, 3])
    g, gl = rng.standard_normal((B, n)), rng.standard_normal((B, 2 * n))
    A, _ = BO.dense(lb, ub)
    got = BD.backward_batch(H, x, mask, g, gl)
    worst = 0.0
    for i in range(B):
        dm = BO.dense_mask(mask[i])
        gH, gf, _, gb = DO.backward(H[i], x[i], lam[i], A[i], dm, g[i], gl[i])
        ref = {"H": gH, "f": gf, "ub": gb[:n], "lb": -gb[n:]}
        for k in BO.NAMES:
            worst = max(worst, float(rel(got[k][i][None], ref[k][None])[0]))
        # dx is the prescribed one on the fixed variables, exactly
        fixed = mask[i, :n] | mask[i, n:]
        assert np.array_equal(got["f"][i][fixed], BD.prescribed(mask[i], gl[i])[fixed])
    fixed = (mask[:, :n] | mask[:, n:]).sum(axis=1)
    print(f"n={n}: fixed {fixed.min()}..{fixed.max()} worst disagreement {worst:.2e}")
    assert worst <= AGREE_TOL
    assert np.array_equal(got["H"], got["H"].transpose(0, 2, 1))
    assert (got["ub"][~mask[:, :n]] == 0.0).all() and (got["lb"][~mask[:, n:]] == 0.0).all()
    # glam where it is not read may hold anything
    ignored = ~BO.dense_mask(mask)
    again = BD.backward_batch(H, x, mask, g, np.where(ignored, np.nan, gl))
    assert all(np.array_equal(again[k], got[k]) for k in BO.NAMES)
    # glam = 0 is box_bwd_oracle.backward
    plain = BO.backward_batch(H, x, mask, g)
    zero = BD.backward_batch(H, x, mask, g, np.zeros((B, 2 * n)))
    assert all(np.array_equal(zero[k], plain[k]) for k in BO.NAMES)


def test_hand_made_masks():
    n = 3
    H = np.array([[2.0, 1.0, 0.0], [1.0, 2.0, 1.0], [0.0, 1.0, 2.0]])
    x, g = np.array([1.0, -1.0, 0.5]), np.array([1.0, 2.0, 3.0])
    gl = np.array([0.5, -0.25, 4.0, np.nan, 8.0, 16.0])
    # variable 0: both bits (the upper counts, the lower glam is NaN); 1: lower; 2: upper
    mask = np.array([1, 0, 1, 1, 1, 0], bool)
    gH, gf, glb, gub = BD.backward(H, x, mask, g, gl)
    d = np.array([-0.5, 8.0, -4.0])
    assert np.array_equal(gf, d) and np.array_equal(gH, 0.5 * (np.outer(d, x) + np.outer(x, d)))
    r = g + H @ d
    assert np.array_equal(gub, [r[0], 0.0, r[2]]) and np.array_equal(glb, [0.0, r[1], 0.0])
    # none fixed: glam is wholly ignored
    out = BD.backward(H, x, np.zeros(2 * n, bool), g, np.full(2 * n, np.nan))
    ref = BO.backward(H, x, np.zeros(2 * n, bool), g)
    assert all(np.array_equal(a, b) for a, b in zip(out, ref))


@pytest.mark.parametrize("n", SIZES)
def test_tangent_against_central_differences(n):
    Bq = 8
    H, f, lb, ub = BO.family(SEED, Bq, n, 10.0)
    x, lam, mask = BO.solve(H, f, lb, ub)
    rng = np.random.default_rng([SEED, n, 4])
    df, dlb, dub = (rng.standard_normal((Bq, n)) for _ in range(3))
    xp, lp, mp = BO.solve(H, f + EPS * df, lb + EPS * dlb, ub + EPS * dub)
    xm, lm, mm = BO.solve(H, f - EPS * df, lb - EPS * dlb, ub - EPS * dub)
    assert np.array_equal(mp, mask) and np.array_equal(mm, mask), "the step changed an active set"
    fd_x, fd_l = (xp - xm) / (2 * EPS), (lp - lm) / (2 * EPS)
    for i in range(Bq):
        dx, dl = BD.tangent(H[i], mask[i], df[i], dlb[i], dub[i])
        assert rel(dx[None], fd_x[i][None])[0] <= FD_TOL, (i, "dx")
        assert rel(dl[None], fd_l[i][None])[0] <= FD_TOL, (i, "dlam")
        assert (dl[~mask[i]] == 0.0).all()
    # the bounds at rest: the tangent along df alone
    dx, dl = BD.tangent(H[0], mask[0], df[0])
    xp, lp, _ = BO.solve(H[:1], f[:1] + EPS * df[:1], lb[:1], ub[:1])
    xm, lm, _ = BO.solve(H[:1], f[:1] - EPS * df[:1], lb[:1], ub[:1])
    assert rel(dx[None], (xp - xm) / (2 * EPS))[0] <= FD_TOL and rel(dl[None], (lp - lm) / (2 * EPS))[0] <= FD_TOL
