"""The oracle of qpb_solve_backward_dual (tests/dual_oracle.py) on the CPU.

  * with glam = 0 it is tests/kkt_oracle.py, bit for bit;
  * K is symmetric, so two right-hand sides and their solutions are reciprocal:
    <(g1, gl1), (dx2, dlam2)> = <(g2, gl2), (dx1, dlam1)>.  Bar 1e-10 relative to
    the two sides' magnitudes: two dense fp64 solves at cond(K) <= ~1e4 agree to
    1e-12 or so;
  * the tangent matches a central difference (eps = 1e-6) of the forward oracle
    eq_oracle.eq_solve in (f, b), for x and for lam.  Bar 1e-4 relative, the
    constants of tests/test_gpu_autograd.py: strict complementarity keeps the
    active set fixed at +-eps.  A moved equality right-hand side moves the
    oracle's feasible start xc with it (by the minimum-norm step).
"""
import numpy as np
import pytest

import dual_oracle as DO
import eq_oracle as EO
import kkt_oracle as KO

EPS = 1e-6
COUNT = 4
SHAPES = [(3, 5, 1), (5, 9, 2), (16, 32, 4), (16, 32, 16), (20, 40, 4)]


def _solved(n, m, meq):
    H, f, A, b, xc = EO.eq_family(11, COUNT, n, m, meq)
    res = [EO.eq_solve(H[i], f[i], A[i], b[i], meq, xc[i]) for i in range(COUNT)]
    assert all(r.status == 0 for r in res)
    return H, f, A, b, xc, res


@pytest.mark.parametrize("n,m,meq", SHAPES + [(3, 0, 0)])
def test_zero_glam_is_the_backward_oracle_bit_for_bit(n, m, meq):
    H, f, A, b, xc = KO.family(11, COUNT, n, m, meq)
    rng = np.random.default_rng(5 + n)
    for i in range(COUNT):
        r = EO.eq_solve(H[i], f[i], A[i], b[i], meq, xc[i]) if m else None
        x = r.x if m else np.linalg.solve(H[i], -f[i])
        lam, act = (r.lam, r.active) if m else (None, None)
        g = rng.standard_normal(n)
        ref = KO.backward(H[i], x, lam, A[i], act, g)
        got = DO.backward(H[i], x, lam, A[i], act, g, np.zeros(m))
        for a, e in zip(got, ref):
            assert np.array_equal(a.view(np.uint8), e.view(np.uint8))
        assert DO.certificate(H[i], A[i], act, g, np.zeros(m), got[1], got[3]) == \
            KO.certificate(H[i], A[i], act, g, got[1], got[3])


@pytest.mark.parametrize("n,m,meq", SHAPES)
def test_reciprocity_and_certificate(n, m, meq):
    H, f, A, b, xc, res = _solved(n, m, meq)
    rng = np.random.default_rng(9 + n)
    for i, r in enumerate(res):
        W = r.active
        g1, g2 = rng.standard_normal(n), rng.standard_normal(n)
        l1, l2 = rng.standard_normal(m), rng.standard_normal(m)
        l1[~W] = np.nan  # never read outside W
        _, dx1, _, gb1 = DO.backward(H[i], r.x, r.lam, A[i], W, g1, l1)
        _, dx2, _, gb2 = DO.backward(H[i], r.x, r.lam, A[i], W, g2, l2)
        assert (gb1[~W] == 0.0).all() and np.isfinite(dx1).all()
        lhs = g1 @ dx2 + l1[W] @ -gb2[W]
        rhs = g2 @ dx1 + l2[W] @ -gb1[W]
        assert abs(lhs - rhs) <= 1e-10 * (1.0 + abs(lhs) + abs(rhs)), (lhs, rhs)
        stat, prim = DO.certificate(H[i], A[i], W, g1, l1, dx1, gb1)
        assert stat <= 1e-12 and prim <= 1e-12, (stat, prim)


@pytest.mark.parametrize("n,m,meq", SHAPES)
def test_tangent_matches_a_central_difference(n, m, meq):
    H, f, A, b, xc, res = _solved(n, m, meq)
    rng = np.random.default_rng(13 + n)
    worst = 0.0
    for i, r in enumerate(res):
        df, db = rng.standard_normal(n), rng.standard_normal(m)
        dx, dlam = DO.tangent(H[i], A[i], r.active, df, db)
        assert (dlam[~r.active] == 0.0).all()
        # the identity qpb.solve_tangent states: one backward with gx = df, glam = -db
        _, gf, _, gb = DO.backward(H[i], r.x, r.lam, A[i], r.active, df, -db)
        assert np.allclose(dx, gf, rtol=0, atol=1e-12 * (1 + np.abs(dx).max()))
        assert np.allclose(dlam, -gb, rtol=0, atol=1e-12 * (1 + np.abs(dlam).max()))
        step = np.linalg.pinv(A[i][:meq]) @ db[:meq] if meq else np.zeros(n)
        side = []
        for s in (EPS, -EPS):
            p = EO.eq_solve(H[i], f[i] + s * df, A[i], b[i] + s * db, meq, xc[i] + s * step)
            assert p.status == 0 and np.array_equal(p.active, r.active)
            side.append(p)
        nx = (side[0].x - side[1].x) / (2 * EPS)
        nl = (side[0].lam - side[1].lam) / (2 * EPS)
        worst = max(worst, np.abs(dx - nx).max() / (1.0 + np.abs(nx).max()),
                    np.abs(dlam - nl).max() / (1.0 + np.abs(nl).max()))
    print(f"({n},{m},{meq}): worst |tangent - central difference| / (1 + |cd|) = {worst:.2e}")
    assert worst <= 1e-4
