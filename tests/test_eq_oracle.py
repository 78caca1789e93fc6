"""CPU tests of tests/eq_oracle.py, the checker of qpb_solve_eq: its answers
pass its own mixed KKT certificate, it is oracle.active_set_solve at meq = 0,
and it agrees with that solver on an equality written as two inequalities."""
import numpy as np
import pytest

import eq_oracle as EO
import oracle as O

# (n, m, meq): the shapes of tests/test_gpu_eq.py's parity test
SHAPES = [(16, 32, 4), (16, 32, 1), (16, 32, 15), (16, 32, 16), (16, 16, 3), (7, 13, 3), (1, 2, 1),
          (16, 33, 5), (20, 33, 5), (32, 64, 8), (32, 64, 32)]
B = 67
KKT_TOL = 1e-9


@pytest.mark.parametrize("n,m,meq", SHAPES)
def test_certificate(n, m, meq):
    H, f, A, b, xc, refs = EO.eq_reference(11 + n + meq, B, n, m, meq)
    x = np.array([r.x for r in refs])
    lam = np.array([r.lam for r in refs])
    worst = {k: float(v.max()) for k, v in EO.kkt_mixed(H, f, A, b, meq, x, lam).items()}
    print((n, m, meq), worst)
    assert all(v <= KKT_TOL for v in worst.values()), worst
    assert all(r.active[:meq].all() for r in refs)
    if meq == n:  # nothing is left to choose: x = xc, no inequality active
        assert np.array_equal(x, xc) and not np.array([r.active[meq:] for r in refs]).any()


def test_certificate_sees_a_wrong_answer():
    """The certificate is not vacuous: moving x off the equalities, or flipping
    an inequality multiplier's sign, fails it."""
    n, m, meq = 7, 13, 3
    H, f, A, b, xc, refs = EO.eq_reference(11 + n + meq, B, n, m, meq)
    x = np.array([r.x for r in refs])
    lam = np.array([r.lam for r in refs])
    assert EO.kkt_mixed(H, f, A, b, meq, x + 1e-3, lam)["prim"].max() > 1e-6
    j = int(np.argmax(lam[:, meq:].max(axis=1)))
    bad = lam.copy()
    bad[j, meq:] *= -1.0
    assert EO.kkt_mixed(H[j:j + 1], f[j:j + 1], A[j:j + 1], b[j:j + 1], meq, x[j:j + 1], bad[j:j + 1])["dual"][0] > 1e-3


def test_meq_zero_is_active_set_solve():
    H, f, A, b, xc = O.family_shifted(5, 9, 7, 13)
    for i in range(len(f)):
        got = EO.eq_solve(H[i], f[i], A[i], b[i], 0, xc[i])
        want = O.active_set_solve(H[i], f[i], A[i], b[i], x0=xc[i])
        assert np.array_equal(got.x, want.x) and np.array_equal(got.lam, want.lam)
        assert np.array_equal(got.active, want.active)


def test_two_inequality_rewrite():
    """n = 4: a x = d written as a x <= d, -a x <= -d.  The helper's answer with
    lam+ = max(lam_eq, 0), lam- = max(-lam_eq, 0) passes the unchanged
    oracle.kkt_residuals on the rewritten QP, which is strictly convex, so its
    KKT point is unique: the same x.  And oracle.active_set_solve on the
    rewrite gives that x and lam_eq = lam+ - lam- wherever it finishes: the
    primal method is not reliable on the dependent pair (every feasible point
    is degenerate; of these 12 QPs it leaves QP 7 infeasible by 0.12), so its
    answer is compared where it passes the certificate, at least 10 of 12."""
    n, m, meq = 4, 8, 2
    H, f, A, b, xc = EO.eq_family(3, 12, n, m, meq)
    A2 = np.concatenate([A, -A[:, :meq]], axis=1)
    b2 = np.concatenate([b, -b[:, :meq]], axis=1)
    got = [EO.eq_solve(H[i], f[i], A[i], b[i], meq, xc[i]) for i in range(len(f))]
    x = np.array([r.x for r in got])
    lam = np.array([r.lam for r in got])
    lam2 = np.concatenate([np.maximum(lam[:, :meq], 0.0), lam[:, meq:], np.maximum(-lam[:, :meq], 0.0)], axis=1)
    worst = {k: float(v.max()) for k, v in O.kkt_residuals(H, f, A2, b2, x, lam2).items()}
    assert all(v <= 1e-9 for v in worst.values()), worst
    compared = 0
    for i in range(len(f)):
        want = O.active_set_solve(H[i], f[i], A2[i], b2[i], x0=xc[i])
        cert = O.kkt_residuals(H[i:i + 1], f[i:i + 1], A2[i:i + 1], b2[i:i + 1], want.x[None], want.lam[None])
        if want.status != 0 or max(float(v[0]) for v in cert.values()) > 1e-9:
            continue
        compared += 1
        assert np.abs(got[i].x - want.x).max() <= 1e-9 * max(1.0, np.abs(want.x).max())
        lam_eq = want.lam[:meq] - want.lam[m:]
        assert np.abs(got[i].lam[:meq] - lam_eq).max() <= 1e-8 * (1.0 + np.abs(lam_eq).max())
        assert np.array_equal(got[i].active[meq:], want.active[meq:m])
    assert compared >= 10, compared
