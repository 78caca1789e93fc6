"""qpb_factor_box + qpb_solve_box_factored on the GPU: the one H of a batch of
box QPs factored once.  The contract is qpb_solve_box_shared's on the H the
buffer was made from, minus bit-for-bit equality: x and lam may differ by
rounding, iters may differ, status and active are the same on a strictly
complementary QP.  Held against qpb_solve_box_shared on the same inputs and
against the CPU oracle (box_bwd_oracle.solve) on tests/box_shared_harness.py's
family at n in {1, 5, 16} (gi_box padded and N16) and {17, 20, 32} (gi_wave's
BOX form), B in {1, 5, 67}; with absent, infinite, NaN, pinned and crossed
bounds, capped iterations, a NaN in one f, a non-SPD and a NaN H0; and for what
a buffer promises: a QP's bits do not depend on its batch or position, the
buffer is only read, any number of solves on any streams may share it, and a
solve queued behind the factorisation needs no host synchronisation.  Every
call goes through the C-ABI into buffers filled with 0xA5 and fenced by guard
words (tests/box_factored_cases.py): every element is written, nothing outside.

Measured on one MI355X (the parity test prints it; not asserted beyond the 1e-6
bar): over the 18 cases the worst relative difference between the factored and
the unfactored x is 2.4e-13 (n = 32, B = 67; 1.3e-13 at n = 16, 2.2e-13 at
n = 20), against the oracle 3.3e-13, the worst KKT residual 2.1e-13, and iters
differs on none of the 438 QPs -- README.md, "Box solves on an H factored once".
"""
import numpy as np
import pytest

import box_factored_cases as C
import box_shared_harness as BH

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

OK, MAX_ITER, NOT_SPD, INFEASIBLE, NUMERICAL = 0, 1, 2, 3, 4
EDGE_N = (5, 16, 20, 32)  # gi_box padded and N16, gi_wave's BOX form below and at its padded size
EDGE_B = 67
PER = lambda n: {"x": n, "lam": 2 * n, "active": (2 * n + 31) // 32, "status": 1, "iters": 1}  # noqa: E731


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    return q


_FAC = {}


def _factor(qpb, n, B=EDGE_B):
    """The buffer of BH.family(B, n)'s H0: made once per case, shared, only read."""
    if (B, n) not in _FAC:
        _FAC[(B, n)] = C.factor(qpb, BH.family(B, n)[0])
        assert C.factor_result(_FAC[(B, n)])[1] == OK
    return _FAC[(B, n)]


def _rows(out, n, keep):
    """The outputs of the QPs in `keep`, one flat array per name."""
    B = len(out["status"])
    return {k: np.ascontiguousarray(out[k].reshape(B, w)[keep]) for k, w in PER(n).items() if k in out}


def _promises(H0, f, out, n, max_iter=None):
    """What qpb.h promises of every QP whatever its status: lam >= 0 exactly and
    zero outside `active`; stationarity with the lam as written wherever x is
    specified; zeroed outputs for a finding of the set-up."""
    st, it, lam, x = out["status"], out["iters"], out["lam"], out["x"]
    mask = C.mask_of(out["active"], n)
    setup = (st == NOT_SPD) | ((it == 0) & ((st == INFEASIBLE) | (st == NUMERICAL)))
    assert (lam[setup] == 0).all() and not mask[setup].any() and (it[setup] == 0).all()
    fin = np.isfinite(lam).all(axis=1)
    assert fin[np.isfinite(f).all(axis=1)].all()
    assert (lam[fin] >= 0).all() and (lam[fin][~mask[fin]] == 0).all()
    spec = ~setup & np.isfinite(x).all(axis=1) & np.isfinite(f).all(axis=1)
    r = x[spec] @ H0.T + f[spec] + lam[spec][:, :n] - lam[spec][:, n:]
    sc = 1.0 + np.abs(f[spec]).max(axis=1) + np.abs(H0).sum(axis=1).max() * np.abs(x[spec]).max(axis=1)
    assert spec.sum() == 0 or (np.abs(r).max(axis=1) <= C.KKT_TOL * sc).all()
    if max_iter is not None:
        assert (it[st == MAX_ITER] == max_iter).all() and (it <= max_iter).all()


@pytest.mark.parametrize("B", C.BATCHES)
@pytest.mark.parametrize("n", C.NS)
def test_parity_with_the_unfactored_solve_and_the_oracle(qpb, n, B):
    H0, f, lb, ub = BH.family(B, n)
    xo, lo, ao, strict = C.oracle(B, n)
    assert strict.mean() >= C.MIN_STRICT_SHARE  # a condition on the inputs
    F = C.factor(qpb, H0)
    fac, fst = C.factor_result(F)
    assert fst == OK and fac[0] == 0.0 and fac[1] == n and fac[2] == (16 if n <= 16 else 32)
    assert len(fac) == qpb.factor_box_doubles(n)
    got = C.solve(qpb, F, f, lb, ub)
    ref = C.shared(qpb, H0, f, lb, ub)
    assert np.array_equal(got["status"], ref["status"]) and (got["status"] == OK).all()
    dx, dxo = C.relx(got["x"], ref["x"]).max(), C.relx(got["x"], xo).max()
    dl, dlo = C.rell(got["lam"], ref["lam"]).max(), C.rell(got["lam"], lo).max()
    res = C.kkt(H0, f, lb, ub, got["x"], got["lam"])
    differ = int((got["iters"] != ref["iters"]).sum())
    print(f"n={n} B={B}: x vs unfactored {dx:.3g}, vs oracle {dxo:.3g}; lam {dl:.3g}, {dlo:.3g}; KKT {res:.3g}; "
          f"iters differ on {differ} of {B} QPs")
    assert max(dx, dxo) <= C.X_TOL and max(dl, dlo) <= C.LAM_TOL
    assert res <= C.KKT_TOL
    assert (got["lam"] >= 0).all()
    mg, mr = C.mask_of(got["active"], n), C.mask_of(ref["active"], n)
    assert np.array_equal(mg[strict], mr[strict]) and np.array_equal(mg[strict], ao[strict])
    assert C.factor_result(F)[0].tobytes() == fac.tobytes()  # the solve only read the buffer


@pytest.mark.parametrize("n", EDGE_N)
def test_absent_bounds(qpb, n):
    H0, f, lb, ub = BH.family(EDGE_B, n)
    F = _factor(qpb, n)
    for lo, up in ((None, ub), (lb, None), (None, None)):
        got, ref = C.solve(qpb, F, f, lo, up), C.shared(qpb, H0, f, lo, up)
        assert np.array_equal(got["status"], ref["status"]) and (got["status"] == OK).all()
        assert C.relx(got["x"], ref["x"]).max() <= C.X_TOL and C.rell(got["lam"], ref["lam"]).max() <= C.LAM_TOL
        assert C.kkt(H0, f, lo, up, got["x"], got["lam"]) <= C.KKT_TOL
        assert np.array_equal(C.mask_of(got["active"], n), C.mask_of(ref["active"], n))
        half = got["lam"][:, n:] if lo is None else got["lam"][:, :n]
        assert (half == 0).all()  # an absent side carries no multiplier
        _promises(H0, f, got, n)
    x0 = np.linalg.solve(H0, -f.T).T  # both NULL: the unconstrained minimiser
    assert C.relx(got["x"], x0).max() <= C.X_TOL and (got["lam"] == 0).all()
    assert np.array_equal(got["iters"], ref["iters"])


@pytest.mark.parametrize("n", EDGE_N)
def test_infinite_nan_pinned_and_crossed_bounds(qpb, n):
    B = EDGE_B
    H0, f, lb, ub = BH.family(B, n)
    F = _factor(qpb, n)
    lb, ub = lb.copy(), ub.copy()
    j = np.arange(B) % n
    q = np.arange(B)
    ub[q[0::5], j[0::5]] = np.inf
    lb[q[1::5], j[1::5]] = -np.inf
    ub[q[2::5], j[2::5]] = np.nan
    lb[q[3::5], j[3::5]] = np.nan
    pin = q[4::5]
    ub[pin, j[pin]] = lb[pin, j[pin]]  # pinned: lb = ub
    got, ref = C.solve(qpb, F, f, lb, ub), C.shared(qpb, H0, f, lb, ub)
    assert np.array_equal(got["status"], ref["status"]) and (got["status"] == OK).all()
    assert C.relx(got["x"], ref["x"]).max() <= C.X_TOL
    assert C.kkt(H0, f, lb, ub, got["x"], got["lam"]) <= C.KKT_TOL
    _promises(H0, f, got, n)
    absent = ~np.isfinite(np.concatenate([ub, -lb], axis=1))
    assert (got["lam"][absent] == 0).all() and not C.mask_of(got["active"], n)[absent].any()
    # a pinned variable sits on its bound, and lam_ub - lam_lb is its one multiplier (stationarity, above)
    assert (np.abs(got["x"][pin, j[pin]] - lb[pin, j[pin]]) <= 1e-9 * (1.0 + np.abs(lb[pin, j[pin]]))).all()
    one = got["lam"][pin, j[pin]] - got["lam"][pin, n + j[pin]]
    oner = ref["lam"][pin, j[pin]] - ref["lam"][pin, n + j[pin]]
    assert (np.abs(one - oner) <= C.LAM_TOL * (1.0 + np.abs(ref["lam"][pin]).max(axis=1))).all()
    # crossed bounds on every third QP: lb > ub on one variable
    lb2, ub2 = BH.family(B, n)[2].copy(), BH.family(B, n)[3].copy()
    lb2[::3, 0], ub2[::3, 0] = ub2[::3, 0] + 1.0, lb2[::3, 0] - 1.0
    got, ref = C.solve(qpb, F, f, lb2, ub2), C.shared(qpb, H0, f, lb2, ub2)
    assert np.array_equal(got["status"], ref["status"])
    assert (got["status"][::3] != OK).all() and (np.delete(got["status"], np.s_[::3]) == OK).all()
    _promises(H0, f, got, n)
    ok = got["status"] == OK
    assert C.relx(got["x"][ok], ref["x"][ok]).max() <= C.X_TOL


@pytest.mark.parametrize("n", EDGE_N)
@pytest.mark.parametrize("max_iter", [1, 3])
def test_capped_iterations(qpb, n, max_iter):
    B = EDGE_B
    H0, f, lb, ub = BH.family(B, n)
    F = _factor(qpb, n)
    full = C.solve(qpb, F, f, lb, ub)
    got = C.solve(qpb, F, f, lb, ub, max_iter=max_iter)
    need = full["iters"]
    assert np.array_equal(got["status"] == MAX_ITER, need > max_iter) and (got["status"] <= MAX_ITER).all()
    assert (got["status"] == MAX_ITER).any()
    _promises(H0, f, got, n, max_iter=max_iter)
    # a QP that needs <= max_iter iterations: the uncapped solve bit for bit
    fits = need <= max_iter
    assert BH.same(_rows(got, n, fits), _rows(full, n, fits))


@pytest.mark.parametrize("n", EDGE_N)
def test_nan_in_one_f_leaves_the_other_qps_alone(qpb, n):
    B = EDGE_B
    H0, f, lb, ub = BH.family(B, n)
    F = _factor(qpb, n)
    clean = C.solve(qpb, F, f, lb, ub)
    f = f.copy()
    bad = 9  # the second QP of its wavefront at n <= 16
    f[bad, n // 2] = np.nan
    got = C.solve(qpb, F, f, lb, ub)
    assert got["status"][bad] != OK
    keep = np.arange(B) != bad
    assert BH.same(_rows(got, n, keep), _rows(clean, n, keep))


@pytest.mark.parametrize("n", EDGE_N)
def test_non_spd_and_nan_h0(qpb, n):
    B = EDGE_B
    H0, f, lb, ub = BH.family(B, n)
    bad = []
    Hn = H0.copy()
    Hn[n - 1, n - 1] = -1.0  # indefinite
    bad.append(Hn)
    Hn = H0.copy()
    Hn[n // 2, n // 2] = np.nan
    bad.append(Hn)
    Hn = H0.copy()
    Hn[n - 1, 0] = Hn[0, n - 1] = np.nan  # off the diagonal, H still symmetric
    bad.append(Hn)
    for Hn in bad:
        F = C.factor(qpb, Hn)
        fac, fst = C.factor_result(F)
        assert fst == NOT_SPD and fac[0] == float(NOT_SPD)
        got = C.solve(qpb, F, f, lb, ub)
        assert (got["status"] == NOT_SPD).all() and (got["iters"] == 0).all()
        assert (got["lam"] == 0).all() and (got["active"] == 0).all()
        assert (C.shared(qpb, Hn, f, lb, ub)["status"] == NOT_SPD).all()


@pytest.mark.parametrize("n", C.NS)
def test_a_qp_does_not_depend_on_its_batch_or_position(qpb, n):
    B = EDGE_B
    H0, f, lb, ub = BH.family(B, n)
    F = _factor(qpb, n)
    full = C.solve(qpb, F, f, lb, ub)
    for k in (0, 2, 4):
        one = C.solve(qpb, F, f[k:k + 1], lb[k:k + 1], ub[k:k + 1])
        five = C.solve(qpb, F, f[:5], lb[:5], ub[:5])
        assert BH.same(_rows(one, n, [0]), _rows(full, n, [k])), k
        assert BH.same(_rows(five, n, [k]), _rows(full, n, [k])), k
    # ... nor on where it stands: the batch reversed
    rev = C.solve(qpb, F, f[::-1].copy(), lb[::-1].copy(), ub[::-1].copy())
    assert BH.same(_rows(rev, n, np.arange(B)[::-1]), _rows(full, n, np.arange(B)))


@pytest.mark.parametrize("n", [16, 20])
def test_one_buffer_many_solves(qpb, n):
    B = EDGE_B
    H0, f, lb, ub = BH.family(B, n)
    F = C.factor(qpb, H0)
    fac = C.factor_result(F)[0]
    fresh = C.solve(qpb, C.factor(qpb, H0), f, lb, ub)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    # two solves queued on two streams from the one buffer (the Python binding does not synchronise), then a third
    BF = qpb.BoxFactor(F[0][F[1]:F[1] + len(fac)], n, None)
    fd, ld, ud = BH.dev(f), BH.dev(lb), BH.dev(ub)
    torch.cuda.synchronize()
    a = qpb.solve_box_factored(BF, fd, ld, ud, stream=s1)
    b = qpb.solve_box_factored(BF, fd, ld, ud, stream=s2)
    torch.cuda.synchronize()
    third = C.solve(qpb, F, f, lb, ub)
    assert C.factor_result(F)[0].tobytes() == fac.tobytes()  # bitwise unchanged
    assert BH.same(third, fresh)
    for sol in (a, b):
        for k in C.OUT:
            assert BH.bits(getattr(sol, k).cpu().numpy().ravel().view(fresh[k].dtype), fresh[k].ravel()), k


@pytest.mark.parametrize("n", [5, 16, 32])
def test_factor_then_solve_on_a_side_stream_without_a_host_sync(qpb, n):
    B = EDGE_B
    H0, f, lb, ub = BH.family(B, n)
    ref = C.solve(qpb, _factor(qpb, n), f, lb, ub)
    side = torch.cuda.Stream()
    fd, ld, ud = BH.dev(f), BH.dev(lb), BH.dev(ub)
    torch.cuda.synchronize()
    F = C.factor(qpb, H0, stream=side, sync=False)
    got = C.solve(qpb, F, fd, ld, ud, stream=side)
    assert BH.same(got, ref)
    assert C.factor_result(F)[0].tobytes() == C.factor_result(_factor(qpb, n))[0].tobytes()


@pytest.mark.parametrize("n", [16, 20])
def test_iters_and_fstatus_null_change_nothing_else(qpb, n):
    B = EDGE_B
    H0, f, lb, ub = BH.family(B, n)
    ref = C.solve(qpb, _factor(qpb, n), f, lb, ub)
    F = C.factor(qpb, H0, fstatus=False)
    assert C.factor_result(F)[0].tobytes() == C.factor_result(_factor(qpb, n))[0].tobytes()
    got = C.solve(qpb, F, f, lb, ub, iters=False)
    assert "iters" not in got
    assert BH.same(got, {k: v for k, v in ref.items() if k != "iters"})


@pytest.mark.parametrize("n", [5, 16, 20])
def test_host_forms_give_the_device_calls_bits(qpb, n):
    B = 5
    H0, f, lb, ub = BH.family(B, n)
    Fd = C.factor(qpb, H0)
    Fh = C.factor(qpb, H0, host=True)
    fac_d, st_d = C.factor_result(Fd)
    fac_h, st_h = C.factor_result(Fh)
    assert fac_d.tobytes() == fac_h.tobytes() and st_d == st_h == OK
    ref = C.solve(qpb, Fd, f, lb, ub)
    assert BH.same(C.solve(qpb, Fh, f, lb, ub, host=True), ref)
    assert BH.same(C.solve(qpb, Fh, f, None, ub, host=True), C.solve(qpb, Fd, f, None, ub))


def test_python_binding(qpb):
    n, B = 20, 5
    H0, f, lb, ub = BH.family(B, n)
    ref = C.solve(qpb, C.factor(qpb, H0), f, lb, ub)
    F = qpb.factor_box(BH.dev(H0))
    assert F.n == n and tuple(F.fac.shape) == (qpb.factor_box_doubles(n),) and int(F.status.cpu()[0]) == OK
    sol = qpb.solve_box_factored(F, BH.dev(f), BH.dev(lb), BH.dev(ub))
    torch.cuda.synchronize()
    assert sol.x.shape == (B, n) and sol.lam.shape == (B, 2 * n)
    assert BH.bits(sol.x.cpu().numpy(), ref["x"]) and np.array_equal(sol.status.cpu().numpy(), ref["status"])
    out = qpb.solve_box_factored(F, BH.dev(f), BH.dev(lb), BH.dev(ub), out=sol)  # out=: the same tensors, rewritten
    assert out is sol
    hs = qpb.solve_box_factored_host(qpb.factor_box_host(H0), f, lb, ub)
    assert BH.bits(hs.x, ref["x"]) and BH.bits(hs.lam, ref["lam"])
    with pytest.raises(ValueError):
        qpb.factor_box(BH.dev(np.broadcast_to(H0, (B, n, n)).copy()))
    with pytest.raises(ValueError):
        qpb.solve_box_factored(qpb.BoxFactor(F.fac[:-2], n, F.status), BH.dev(f))
    with pytest.raises(qpb.QPBError):
        qpb.factor_box_doubles(33)
