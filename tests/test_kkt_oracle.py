"""The oracle of qpb_solve_backward (tests/kkt_oracle.py) against finite
differences of the forward oracle (tests/eq_oracle.py), on the CPU.

The directional derivative sum(g . dx*) along one seeded direction that moves
all of H (symmetrically), f, A and b is compared with a central difference
(eps = 1e-6) of eq_oracle.eq_solve.  The families have strict complementarity
(active multipliers and inactive slacks >= 6e-3), so the active set is the same
at +-eps.  Bar 1e-4 relative: the agreement measured 3.4e-7 at worst, the
margin covers the noise of a finite difference.  The oracle's own certificate
is <= 1e-12 (measured <= 3e-14, also at meq = n).
"""
import numpy as np
import pytest

import eq_oracle as EO
import kkt_oracle as KO

EPS = 1e-6
COUNT = 4


@pytest.mark.parametrize("n,m,meq", [(3, 5, 1), (16, 32, 4), (20, 40, 4)])
def test_oracle_matches_finite_differences(n, m, meq):
    H, f, A, b, xc = EO.eq_family(11, COUNT, n, m, meq)
    rng = np.random.default_rng(7 + n)
    worst = 0.0
    for i in range(COUNT):
        r = EO.eq_solve(H[i], f[i], A[i], b[i], meq, xc[i])
        assert r.status == 0
        g = rng.standard_normal(n)
        gH, gf, gA, gb = KO.backward(H[i], r.x, r.lam, A[i], r.active, g)
        dH = rng.standard_normal((n, n))
        dH = 0.5 * (dH + dH.T)
        df, dA, db = rng.standard_normal(n), rng.standard_normal((m, n)), rng.standard_normal(m)
        # keep xc on the moved equalities: d(b_eq) = dA_eq xc along the direction
        db[:meq] = dA[:meq] @ xc[i]
        ana = (gH * dH).sum() + gf @ df + (gA * dA).sum() + gb @ db
        xp = EO.eq_solve(H[i] + EPS * dH, f[i] + EPS * df, A[i] + EPS * dA, b[i] + EPS * db, meq, xc[i])
        xm = EO.eq_solve(H[i] - EPS * dH, f[i] - EPS * df, A[i] - EPS * dA, b[i] - EPS * db, meq, xc[i])
        assert np.array_equal(xp.active, r.active) and np.array_equal(xm.active, r.active)
        num = g @ (xp.x - xm.x) / (2 * EPS)
        worst = max(worst, abs(ana - num) / (1.0 + abs(num)))
    print(f"({n},{m},{meq}): worst |analytic - central difference| / (1 + |cd|) = {worst:.2e}")
    assert worst <= 1e-4


@pytest.mark.parametrize("n,m,meq", [(3, 5, 1), (16, 32, 4), (16, 32, 16), (20, 40, 4), (3, 0, 0)])
def test_oracle_certificate(n, m, meq):
    H, f, A, b, xc = KO.family(11, COUNT, n, m, meq)
    rng = np.random.default_rng(3)
    for i in range(COUNT):
        r = EO.eq_solve(H[i], f[i], A[i], b[i], meq, xc[i]) if m else None
        x = r.x if m else np.linalg.solve(H[i], -f[i])
        g = rng.standard_normal(n)
        gH, gf, gA, gb = KO.backward(H[i], x, r.lam if m else None, A[i], r.active if m else None, g)
        stat, prim = KO.certificate(H[i], A[i], r.active if m else None, g, gf, gb)
        assert stat <= 1e-12 and prim <= 1e-12, (stat, prim)
        assert np.array_equal(gH, gH.T)
