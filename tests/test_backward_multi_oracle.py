"""CPU tests for the multi-direction KKT solves (no GPU).

What the GPU tests of qpb_solve_factored_backward_multi and
qpb_solve_box_backward_multi lean on: the oracles tests/dual_oracle.py and
tests/box_dual_oracle.py, applied once per direction, equal ONE dense solve of
the KKT matrix with T right-hand-side columns -- the T directions are T columns
of K^-1 applied to a matrix, which is what the calls compute in one launch.  And
the Python wrappers' argument checks that need no device: the direction-major
layouts (B, T, n) / (T, n), T's limits, and the tangents' sign conventions on
the oracle.
"""
import numpy as np
import pytest

import box_dual_oracle as BD
import dual_oracle as DO
from bwd_harness import rel

# a few ulp of the dense solve's own backward error at these well-conditioned sizes: cond(K) <= ~1e3, n + k <= 24
TOL = 1e-10


def _qp(seed, n, m, k):
    rs = np.random.default_rng([seed, n, m, k])
    Bm = rs.standard_normal((n, n))
    H = np.eye(n) + Bm.T @ Bm / n
    A = rs.standard_normal((m, n))
    act = np.zeros(m, bool)
    act[rs.permutation(m)[:k]] = True
    return rs, H, A, act


@pytest.mark.parametrize("n,m,k,T", [(5, 9, 2, 5), (16, 32, 8, 17), (3, 0, 0, 2), (7, 14, 7, 1)])
def test_dual_oracle_per_direction_is_one_solve_with_t_columns(n, m, k, T):
    rs, H, A, act = _qp(31, n, m, k)
    g, gl = rs.standard_normal((T, n)), rs.standard_normal((T, m))
    W = np.flatnonzero(act)
    K = np.block([[H, A[W].T], [A[W], np.zeros((k, k))]])
    X = np.linalg.solve(K, -np.concatenate([g, gl[:, W]], axis=1).T)  # (n + k, T): one solve, T columns
    x, lam = rs.standard_normal(n), rs.standard_normal(m)
    for t in range(T):
        _, gf, _, gb = DO.backward(H, x, lam, A, act, g[t], gl[t])
        assert rel(gf[None], X[:n, t][None])[0] <= TOL
        ref_b = np.zeros(m)
        ref_b[W] = -X[n:, t]
        assert m == 0 or rel(gb[None], ref_b[None])[0] <= TOL
        # the same column read as a tangent: gx = df, glam = -db, dlam = -gb
        dx, dlam = DO.tangent(H, A, act, g[t], -gl[t])
        assert rel(dx[None], gf[None])[0] <= TOL and (m == 0 or rel(dlam[None], -gb[None])[0] <= TOL)
    # the Jacobian dx* / df from gx = I is symmetric and A_W J = 0
    J = np.array([DO.backward(H, x, lam, A, act, e, np.zeros(m))[1] for e in np.eye(n)])
    assert np.abs(J - J.T).max() <= TOL and (k == 0 or np.abs(A[W] @ J.T).max() <= TOL)


@pytest.mark.parametrize("n,T", [(1, 2), (5, 5), (16, 17), (20, 3)])
def test_box_oracle_per_direction_is_one_solve_with_t_columns(n, T):
    rs, H, _, _ = _qp(37, n, 0, 0)
    mask = np.zeros(2 * n, bool)
    mask[rs.permutation(2 * n)[:max(1, n // 2)]] = True
    g, gl = rs.standard_normal((T, n)), rs.standard_normal((T, 2 * n))
    # the explicit rows A = [I; -I] without the lower row of a variable whose both bits are set
    A = np.concatenate([np.eye(n), -np.eye(n)])
    dm = mask.copy()
    dm[n:] &= ~mask[:n]
    W = np.flatnonzero(dm)
    k = len(W)
    K = np.block([[H, A[W].T], [A[W], np.zeros((k, k))]])
    X = np.linalg.solve(K, -np.concatenate([g, gl[:, W]], axis=1).T)
    x = rs.standard_normal(n)
    for t in range(T):
        _, gf, glb, gub = BD.backward(H, x, mask, g[t], gl[t])
        assert rel(gf[None], X[:n, t][None])[0] <= TOL
        gb = np.zeros(2 * n)
        gb[W] = -X[n:, t]
        assert rel(gub[None], gb[:n][None])[0] <= TOL and rel(glb[None], -gb[n:][None])[0] <= TOL
        dx, dlam = BD.tangent(H, mask, g[t], gl[t, n:], -gl[t, :n])
        assert np.array_equal(dx, gf) and np.array_equal(dlam, np.concatenate([-gub, glb]))


def test_python_wrappers_check_layouts_without_a_device():
    import qpb
    B, T, n, m = 4, 3, 5, 6
    hs = qpb.Solution(None, None, np.zeros((B, 1), np.uint32), np.zeros(B, np.int32), None)
    hF = qpb.BackwardFactor(np.zeros(qpb.factor_backward_doubles(n, m)), n, m, None)
    # direction-major right-hand sides: (B, T, n), or (T, n) for one shared set; glam follows gx
    assert qpb._multi_dims(np.zeros((B, T, n)), n, B) == (T, 0)
    assert qpb._multi_dims(np.zeros((T, n)), n, B) == (T, qpb.SHARED_RHS)
    assert qpb._multi_dims(np.zeros((B, 1, n)), n, B) == (1, 0)
    assert qpb._multi_dims(np.zeros((qpb.MAX_RHS, n)), n, B) == (qpb.MAX_RHS, qpb.SHARED_RHS)
    for bad in (np.zeros((T, B, n + 1)), np.zeros((B + 1, T, n)), np.zeros((B, T, n, 1)), np.zeros(n)):
        with pytest.raises(ValueError, match="shape mismatch"):
            qpb._multi_dims(bad, n, B)
    for T_bad in (0, qpb.MAX_RHS + 1):
        with pytest.raises(ValueError, match="right-hand sides"):
            qpb._multi_dims(np.zeros((B, T_bad, n)), n, B)
    # B comes from sol.active, or from sol.status at m == 0
    assert qpb._multi_sol_batch(hs) == B
    assert qpb._multi_sol_batch(qpb.Solution(None, None, None, np.zeros(7, np.int32), None)) == 7
    with pytest.raises(ValueError, match="batch size"):
        qpb._multi_sol_batch(qpb.Solution(None, None, None, None, None))
    with pytest.raises(ValueError, match="shape mismatch"):
        qpb.solve_factored_backward_multi_host(hF, hs, np.zeros((B, T, n)), np.zeros((B, T + 1, m)))
    with pytest.raises(ValueError, match="shape mismatch"):
        qpb.solve_factored_backward_multi_host(hF, hs._replace(status=np.zeros(B + 1, np.int32)), np.zeros((B, T, n)))
    with pytest.raises(ValueError, match="shape mismatch"):
        qpb.solve_box_backward_multi_host(np.zeros((n, n)), hs, np.zeros((T, n)), np.zeros((T, 2 * n - 1)))
    with pytest.raises(ValueError, match="need"):
        qpb.solve_box_backward_multi_host(np.zeros((n, n)), hs, np.zeros((T, n)), need=())
