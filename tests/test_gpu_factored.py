"""qpb_factor_shared and qpb_solve_factored on the GPU: one shared H and A
factored once, every QP solved from the factor.  The reference is the
unfactored path, qpb_solve_shared(shared = H | A), and the CPU oracle
(tests/eq_oracle.py): the factored path is held to the bars qpb_solve_eq is
held to (tests/test_gpu_eq.py), not to bitwise equality -- s = b + D y is formed
from the stored L and D, so x and lam may differ from the unfactored path's by
rounding.  Every call goes through the C-ABI into buffers filled with 0xA5 and
fenced by guard words (tests/factored_cases.py): every element is written and
nothing outside.

Measured on the MI355X (this file's parity test): the worst relative difference
between the two paths' x over all shapes and batches, per QP as
max|dx| / (1 + max|x|), is 9.8e-14 ((16, 32, 4) at B = 67).
"""
import numpy as np
import pytest

import eq_oracle as EO
import factored_cases as FC
import planted as P
import shared_cases as SC

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

OK, MAX_ITER, NOT_SPD, INFEASIBLE, NUMERICAL = 0, 1, 2, 3, 4
CONTRACT_SHAPES = [(16, 32, 4), (20, 40, 4)]  # both classes


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    return q


def _both(qpb, H0, f, A0, b, meq, max_iter=0):
    """(factored outputs, unfactored outputs, fstatus) on the same inputs."""
    F = FC.factor(qpb, H0, A0)
    got = FC.solve(qpb, F, f, b, meq, max_iter=max_iter)
    return got, FC.shared(qpb, H0, f, A0, b, meq, max_iter=max_iter), FC.factor_result(F)[1]


def _kkt(H0, f, A0, b, meq, x, lam):
    B = len(f)
    res = EO.kkt_mixed(SC.expand(H0, B), f, SC.expand(A0, B), b, meq, x, lam)
    return {k: float(v.max()) for k, v in res.items()}


def _stat(H0, f, A0, x, lam):
    """eq_oracle.kkt_mixed's stationarity residual alone (b may hold +inf here)."""
    r = x @ H0.T + f + lam @ A0
    scale = 1.0 + np.abs(f).max(axis=1) + np.abs(H0).sum(axis=1).max() * np.abs(x).max(axis=1)
    return float((np.abs(r).max(axis=1) / scale).max())


# ------------------------------------------------------------------------ parity
@pytest.mark.parametrize("n,m,meq", FC.SHAPES)
def test_parity_with_the_unfactored_path_and_the_oracle(qpb, n, m, meq):
    for B in FC.BATCHES:
        H0, f, A0, b = SC.family(B, n, m, meq)
        xr, lr, ar, strict = FC.oracle(B, n, m, meq)
        assert strict.mean() >= FC.MIN_STRICT_SHARE, (B, strict.mean())
        got, ref, fstatus = _both(qpb, H0, f, A0, b, meq)
        diff = np.abs(got["x"] - ref["x"]).max(axis=1) / (1.0 + np.abs(ref["x"]).max(axis=1))
        worst = _kkt(H0, f, A0, b, meq, got["x"], got["lam"]) if m else {}
        print(f"({n},{m},{meq}) B={B}: status {np.bincount(got['status'], minlength=5).tolist()} "
              f"x err {FC.relx(got['x'], xr).max():.2e} lam err {FC.rell(got['lam'], lr).max():.2e} "
              f"kkt {max(worst.values(), default=0.0):.2e} strict {int(strict.sum())}/{B} "
              f"iters differ {int((got['iters'] != ref['iters']).sum())} "
              f"factored vs unfactored x: worst relative difference {diff.max():.3e}")
        assert fstatus == OK
        assert np.array_equal(got["status"], ref["status"]) and (got["status"] == OK).all(), (B, got["status"])
        assert FC.relx(got["x"], xr).max() <= FC.X_TOL, B
        assert FC.rell(got["lam"], lr).max() <= FC.LAM_TOL, B
        assert all(v <= FC.KKT_TOL for v in worst.values()), (B, worst)
        assert (got["lam"][:, meq:] >= 0).all(), B
        assert np.array_equal(got["active"][strict], ref["active"][strict]), B
        if m:
            mask = qpb.active_mask_to_bool(got["active"], m)
            assert np.array_equal(mask[strict][:, meq:], ar[strict][:, meq:]) and mask[:, :meq].all(), B
        if m == 0:  # stationarity of the unconstrained minimiser
            assert _stat(H0, f, A0, got["x"], got["lam"]) <= FC.KKT_TOL


# --------------------------------------------------------------- status contract
def _contract(qpb, H0, f, A0, b, meq, max_iter=0):
    got, ref, fstatus = _both(qpb, H0, f, A0, b, meq, max_iter=max_iter)
    assert np.array_equal(got["status"], ref["status"]), (got["status"], ref["status"])
    return got, ref, fstatus


def _zeroed(got, rows):
    """What qpb.h promises for a failure found in the set-up."""
    assert (got["iters"][rows] == 0).all() and (got["lam"][rows] == 0).all() and (got["active"][rows] == 0).all()


@pytest.mark.parametrize("n,m,meq", CONTRACT_SHAPES)
def test_status_contract(qpb, n, m, meq):
    B = 67
    H0, f, A0, b = SC.family(B, n, m, meq)
    every = np.arange(B)
    # an indefinite H: every QP NOT_SPD, and the factor says so
    Hn = H0.copy()
    Hn[n // 2, n // 2] = -1.0
    got, _, fstatus = _contract(qpb, Hn, f, A0, b, meq)
    assert fstatus == NOT_SPD and (got["status"] == NOT_SPD).all()
    _zeroed(got, every)
    # a NaN in one row of A: every QP NUMERICAL (found in the set-up)
    An = A0.copy()
    An[m - 3, 1] = np.nan
    got, _, fstatus = _contract(qpb, H0, f, An, b, meq)
    assert fstatus == NUMERICAL and (got["status"] == NUMERICAL).all()
    _zeroed(got, every)
    # a zero row of A is judged against each QP's own b: b < 0 in some QPs only
    Az, bz = A0.copy(), b.copy()
    Az[m - 1] = 0.0
    bz[:, m - 1] = 1.0
    bz[::3, m - 1] = -1.0
    got, ref, fstatus = _contract(qpb, H0, f, Az, bz, meq)
    bad = np.zeros(B, bool)
    bad[::3] = True
    assert fstatus == OK and (got["status"][bad] == INFEASIBLE).all() and (got["status"][~bad] == OK).all()
    _zeroed(got, bad)
    assert FC.relx(got["x"][~bad], ref["x"][~bad]).max() <= FC.X_TOL
    # a NaN b in a row >= meq: the row is absent, exactly as b = +inf
    bn, bi = b.copy(), b.copy()
    bn[1::5, meq] = np.nan
    bi[1::5, meq] = np.inf
    F = FC.factor(qpb, H0, A0)
    gn, gi = FC.solve(qpb, F, f, bn, meq), FC.solve(qpb, F, f, bi, meq)
    assert all(np.array_equal(gn[k].view(np.uint8), gi[k].view(np.uint8)) for k in FC.OUT)
    assert np.array_equal(gn["status"], FC.shared(qpb, H0, f, A0, bn, meq)["status"]) and (gn["status"] == OK).all()
    assert not qpb.active_mask_to_bool(gn["active"], m)[1::5, meq].any()
    assert _stat(H0, f, A0, gn["x"], gn["lam"]) <= FC.KKT_TOL and (gn["lam"][:, meq:] >= 0).all()
    # a non-finite b on an equality: NUMERICAL from the set-up, in those QPs only
    be = b.copy()
    be[2::7, 0] = np.inf
    be[3::7, 1] = np.nan
    got, _, _ = _contract(qpb, H0, f, A0, be, meq)
    bad = np.zeros(B, bool)
    bad[2::7] = bad[3::7] = True
    assert (got["status"][bad] == NUMERICAL).all() and (got["status"][~bad] == OK).all()
    _zeroed(got, bad)
    # max_iter = 2: MAX_ITER with iters == 2, lam >= 0 off the equalities, zero outside the
    # mask, and x stationary for that lam
    got, _, _ = _contract(qpb, H0, f, A0, b, meq, max_iter=2)
    capped = got["status"] == MAX_ITER
    assert capped.any() and (got["iters"][capped] == 2).all() and (got["status"][~capped] == OK).all()
    mask = qpb.active_mask_to_bool(got["active"], m)
    assert (got["lam"][:, meq:] >= 0).all() and (got["lam"][~mask] == 0).all()
    assert _kkt(H0, f, A0, b, meq, got["x"], got["lam"])["stat"] <= FC.KKT_TOL
    # an infeasible pair of rows, found by the iteration: an empty slab on every third QP
    Ap, bp = A0.copy(), b.copy()
    Ap[m - 1] = -Ap[m - 2]
    bp[:, m - 1] = -bp[:, m - 2] + 1.0
    bp[::3, m - 1] = -bp[::3, m - 2] - 1.0
    got, ref, _ = _contract(qpb, H0, f, Ap, bp, meq)
    bad = np.zeros(B, bool)
    bad[::3] = True
    assert (got["status"][bad] == INFEASIBLE).all() and (got["status"][~bad] == OK).all()
    assert (got["iters"][bad] >= 1).all() and (got["iters"][bad] <= 4 * (n + m) + 8).all()
    mask = qpb.active_mask_to_bool(got["active"], m)
    assert (got["lam"][:, meq:] >= 0).all() and (got["lam"][~mask] == 0).all()
    assert _kkt(H0, f, Ap, bp, meq, got["x"], got["lam"])["stat"] <= FC.KKT_TOL
    assert FC.relx(got["x"][~bad], ref["x"][~bad]).max() <= FC.X_TOL


# -------------------------------------------------- written, and nothing else
@pytest.mark.parametrize("n,m,meq", [(5, 9, 2), (16, 32, 4), (3, 0, 0), (20, 40, 4)])
def test_iters_null_is_accepted_and_changes_nothing(qpb, n, m, meq):
    B = 5  # (FC.solve checks the guards and that every element is written, on every call of this file)
    H0, f, A0, b = SC.family(B, n, m, meq)
    F = FC.factor(qpb, H0, A0)
    fac, fstatus = FC.factor_result(F)  # every double of the buffer written, its guards intact
    assert fstatus == OK and np.isfinite(fac).all() and fac[0] == 0.0 and (fac[1], fac[2]) == (n, m)
    a = FC.solve(qpb, F, f, b if m else None, meq)
    c = FC.solve(qpb, F, f, b if m else None, meq, iters=False)
    assert "iters" not in c
    assert all(np.array_equal(a[k].view(np.uint8), c[k].view(np.uint8)) for k in c)


# ------------------------------------------------------------------ independence
def _bits(a, k):
    """QP k's part of an output, as bytes."""
    return np.ascontiguousarray(a[k:k + 1]).tobytes()


@pytest.mark.parametrize("n,m,meq", FC.SHAPES)
def test_outputs_do_not_depend_on_batch_or_position(qpb, n, m, meq):
    """QP k bitwise the same alone, at position k of 5 and at position k of 67."""
    H0, f, A0, b = SC.family(67, n, m, meq)
    F = FC.factor(qpb, H0, A0)
    bb = b if m else None
    big = FC.solve(qpb, F, f, bb, meq)
    for k in (0, 3, 4):
        five = FC.solve(qpb, F, f[:5], b[:5] if m else None, meq)
        lo = max(0, k - 2)  # ... and at another position of a batch of 5
        moved = FC.solve(qpb, F, f[lo:lo + 5], b[lo:lo + 5] if m else None, meq)
        one = FC.solve(qpb, F, f[k:k + 1], b[k:k + 1] if m else None, meq)
        for key in FC.OUT:
            assert _bits(one[key], 0) == _bits(big[key], k), (k, key)
            assert _bits(one[key], 0) == _bits(five[key], k), (k, key)
            assert _bits(one[key], 0) == _bits(moved[key], k - lo), (k, key)
    last = FC.solve(qpb, F, f[66:67], b[66:67] if m else None, meq)  # the ragged group's only live row
    assert all(_bits(last[key], 0) == _bits(big[key], 66) for key in FC.OUT)


# ------------------------------------------------------------------------- reuse
@pytest.mark.parametrize("n,m,meq", CONTRACT_SHAPES)
def test_one_factor_serves_many_solves(qpb, n, m, meq):
    H0, f, A0, b = SC.family(67, n, m, meq)
    f2, b2 = f[5:10][::-1].copy(), b[5:10][::-1].copy()  # other QPs of the same H0 and A0
    F = FC.factor(qpb, H0, A0)
    before = FC.factor_result(F)[0].copy()
    first = FC.solve(qpb, F, f, b, meq)
    second = FC.solve(qpb, F, f2, b2, meq)
    again = FC.solve(qpb, F, f, b, meq)
    assert np.array_equal(FC.factor_result(F)[0].view(np.uint8), before.view(np.uint8)), "the solve wrote to fac"
    assert all(np.array_equal(first[k].view(np.uint8), again[k].view(np.uint8)) for k in FC.OUT)
    assert (second["status"] == OK).all()
    assert FC.relx(second["x"], FC.oracle(67, n, m, meq)[0][5:10][::-1]).max() <= FC.X_TOL
    assert all(_bits(second[k], 0) == _bits(first[k], 9) for k in FC.OUT)


@pytest.mark.parametrize("n,m,meq", CONTRACT_SHAPES)
def test_factor_then_solve_on_a_side_stream_without_host_sync(qpb, n, m, meq):
    B = 67
    H0, f, A0, b = SC.family(B, n, m, meq)
    ref = FC.solve(qpb, FC.factor(qpb, H0, A0), f, b, meq)
    side = torch.cuda.Stream()
    fd, bd = FC.dev(f), FC.dev(b)  # uploaded first: nothing below waits on the host
    torch.cuda.synchronize()
    F = FC.factor(qpb, H0, A0, stream=side, sync=False)
    got = FC.solve(qpb, F, fd, bd, meq, stream=side)
    assert all(np.array_equal(got[k].view(np.uint8), ref[k].view(np.uint8)) for k in FC.OUT)
    assert FC.factor_result(F)[1] == OK


# ------------------------------------------------------------------- edge shapes
@pytest.mark.parametrize("n,m,meq", [(3, 0, 0), (20, 0, 0), (16, 32, 0), (20, 40, 0), (16, 9, 9), (16, 16, 16),
                                     (20, 33, 20), (16, 32, 16), (32, 64, 32), (7, 7, 7)])
def test_edge_shapes(qpb, n, m, meq):
    """m = 0, meq = 0, meq = m and meq = n: against the unfactored path and the KKT certificate."""
    B = 5
    H0, f, A0, b = SC.family(B, n, m, meq)
    got, ref, fstatus = _both(qpb, H0, f, A0, b, meq)
    assert fstatus == OK and np.array_equal(got["status"], ref["status"]) and (got["status"] == OK).all()
    assert FC.relx(got["x"], ref["x"]).max() <= FC.X_TOL and FC.rell(got["lam"], ref["lam"]).max() <= FC.LAM_TOL
    if m:
        worst = _kkt(H0, f, A0, b, meq, got["x"], got["lam"])
        assert all(v <= FC.KKT_TOL for v in worst.values()), worst
        assert qpb.active_mask_to_bool(got["active"], m)[:, :meq].all()


# ------------------------------------------------------------- degenerate inputs
_DEGENERATE = [r for r in P.DEGENERATE if r[1] <= 32 and r[2] <= 64 and r[4] == 0]


@pytest.mark.parametrize("route", _DEGENERATE, ids=[r[0] for r in _DEGENERATE])
def test_degenerate_inputs_one_qp_at_a_time(qpb, route):
    """tests/planted.py's weak / dup / vertex cases that fit the factored classes,
    each as a batch of one (a single QP is a shared problem): QPB_OK, the
    planted x within tests/test_gpu_degenerate.py's bar (1e-9), the KKT
    certificate, lam >= 0 and no slack row reported active."""
    name, n, m, B, _ = route
    q, kinds = P.dense_batch(n, m, min(B, 9))
    for i, kind in enumerate(kinds):
        F = FC.factor(qpb, q.H[i], q.A[i])
        got = FC.solve(qpb, F, q.f[i:i + 1], q.b[i:i + 1], 0)
        assert FC.factor_result(F)[1] == OK
        assert got["status"][0] == OK and 1 <= got["iters"][0] <= 4 * (n + m) + 8, (name, i, kind, got["status"])
        ex = np.abs(got["x"][0] - q.x[i]).max() / max(1.0, np.abs(q.x[i]).max())
        assert ex <= 1e-9, (name, i, kind, ex)
        worst = _kkt(q.H[i], q.f[i:i + 1], q.A[i], q.b[i:i + 1], 0, got["x"], got["lam"])
        assert all(v <= FC.KKT_TOL for v in worst.values()), (name, i, kind, worst)
        mask = qpb.active_mask_to_bool(got["active"], m)[0]
        assert (got["lam"] >= 0).all() and (got["lam"][0][~mask] == 0).all() and not (mask & ~q.tight[i]).any()


@pytest.mark.parametrize("n,m,meq,B", P.EQ)
def test_degenerate_inputs_with_equalities(qpb, n, m, meq, B):
    q, kinds = P.eq_batch(n, m, meq, min(B, 6))
    for i, kind in enumerate(kinds):
        got = FC.solve(qpb, FC.factor(qpb, q.H[i], q.A[i]), q.f[i:i + 1], q.b[i:i + 1], meq)
        assert got["status"][0] == OK, (i, kind)
        assert np.abs(got["x"][0] - q.x[i]).max() / max(1.0, np.abs(q.x[i]).max()) <= 1e-9, (i, kind)
        worst = _kkt(q.H[i], q.f[i:i + 1], q.A[i], q.b[i:i + 1], meq, got["x"], got["lam"])
        assert all(v <= FC.KKT_TOL for v in worst.values()), (i, kind, worst)
        mask = qpb.active_mask_to_bool(got["active"], m)[0]
        assert mask[:meq].all() and (got["lam"][0, meq:] >= 0).all() and not (mask & ~q.tight[i]).any()


# ------------------------------------------------------------------- the binding
def test_python_binding(qpb):
    n, m, meq, B = 16, 32, 4, 5
    H0, f, A0, b = SC.family(B, n, m, meq)
    F = qpb.factor_shared(FC.dev(H0), FC.dev(A0))
    assert (F.n, F.m) == (n, m) and tuple(F.fac.shape) == (qpb.factor_doubles(n, m),) and tuple(F.status.shape) == (1,)
    sol = qpb.solve_factored(F, FC.dev(f), FC.dev(b), meq)
    torch.cuda.synchronize()
    ref = FC.solve(qpb, FC.factor(qpb, H0, A0), f, b, meq)
    assert int(F.status.item()) == OK
    assert np.array_equal(sol.x.cpu().numpy(), ref["x"]) and np.array_equal(sol.status.cpu().numpy(), ref["status"])
    # the host forms: the same bits
    Fh = qpb.factor_shared_host(H0, A0)
    assert np.array_equal(Fh.fac.view(np.uint8), F.fac.cpu().numpy().view(np.uint8)) and Fh.status[0] == OK
    hs = qpb.solve_factored_host(Fh, f, b, meq)
    assert np.array_equal(hs.x, ref["x"]) and np.array_equal(hs.lam, ref["lam"])
    # a factor for another shape, and shapes that do not match it
    with pytest.raises(ValueError):
        qpb.solve_factored(F, FC.dev(f[:, :5].copy()), FC.dev(b), meq)
    with pytest.raises(ValueError):
        qpb.solve_factored(F, FC.dev(f), FC.dev(b[:, :9].copy()), meq)
    with pytest.raises(ValueError):
        qpb.solve_factored(qpb.SharedFactor(F.fac, 20, 40, F.status), FC.dev(np.zeros((B, 20))), FC.dev(np.zeros((B, 40))))
    for nn, mm in ((33, 0), (16, 65)):
        with pytest.raises(qpb.QPBError) as e:
            qpb.factor_shared(torch.eye(nn, dtype=torch.float64, device="cuda"),
                              torch.zeros((mm, nn), dtype=torch.float64, device="cuda") if mm else None)
        assert e.value.code == qpb.ERR_UNSUPPORTED
