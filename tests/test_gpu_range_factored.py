"""qpb_solve_range_factored on the GPU: two-sided rows bl <= A x <= bu solved
from a factor buffer of qpb_factor_shared -- the buffer qpb_solve_factored
takes, unchanged.  The references are the unfactored path,
qpb_solve_range(shared = H | A), and the CPU oracle (tests/range_oracle.py: the
pair rewrite through eq_oracle.eq_solve and its two-sided KKT certificate).  The
factored path is held to the bars qpb_solve_range is held to
(tests/test_gpu_range.py: x and lam within 1e-6, certificate <= 1e-9), not to
bitwise equality with the unfactored path -- s = b + D y is formed from the
stored L and D, so x and lam may differ by rounding and `iters` may differ.
`active` and `lower` are compared bit for bit on the strictly complementary QPs.
Every call goes through the C-ABI into buffers filled with 0xA5 and fenced by
guard words (tests/range_factored_cases.py): every element is written and
nothing outside.

Measured on the MI355X (this file's parity test; measurements, not bars): the
worst relative difference between the two paths' x over all shapes and batches,
per QP as max|dx| / (1 + max|x|), is 1.4e-13 ((16, 32, 4) at B = 5), and `iters`
differs on no QP.
"""
import numpy as np
import pytest

import factored_cases as FC
import range_factored_cases as RF
import range_oracle as RO
import shared_cases as SC

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

OK, MAX_ITER, NOT_SPD, INFEASIBLE, NUMERICAL = 0, 1, 2, 3, 4
CONTRACT_SHAPES = [(16, 32, 4), (20, 40, 4)]  # both classes
B = 67
TOL = 1e-10  # the default feas_tol


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    return q


def _both(qpb, H0, f, A0, bl, bu, meq, max_iter=0):
    """(factored outputs, unfactored outputs, fstatus) on the same inputs."""
    F = FC.factor(qpb, H0, A0)
    got = RF.solve(qpb, F, f, bl, bu, meq, max_iter=max_iter)
    return got, RF.unfactored(qpb, H0, f, A0, bl, bu, meq, max_iter=max_iter), FC.factor_result(F)[1]


def _masks(got, m):
    return RO.unpack_bits(got["active"], m), RO.unpack_bits(got["lower"], m)


def _signs_agree(lam, act, low, meq):
    """lower is a subset of active and clear below meq; lam is 0 outside active;
    on the rows >= meq a nonzero lam is negative exactly where the lower bit is set."""
    assert not (low & ~act).any()
    assert not low[:, :meq].any()
    assert (lam[~act] == 0).all()
    li, lo = lam[:, meq:], low[:, meq:]
    nz = li != 0
    assert np.array_equal((li < 0)[nz], lo[nz])


def _strict(A0, bl, bu, meq, x, lam, act):
    """Strict complementarity of a computed solution (range_factored_cases.oracle's
    margins): where it holds, two correct solvers agree on the active set."""
    m = A0.shape[0]
    ax = x @ A0.T
    hu = np.where(np.isfinite(bu), bu, np.inf) if bu is not None else np.full(ax.shape, np.inf)
    hl = np.where(np.isfinite(bl), bl, -np.inf) if bl is not None else np.full(ax.shape, -np.inf)
    fin = lambda v: np.where(np.isfinite(v), np.abs(v), 0.0)  # noqa: E731
    slack = np.minimum(hu - ax, ax - hl)
    ln = 1.0 + np.abs(lam).max(axis=1)
    sc = 1.0 + np.maximum(fin(hu).max(axis=1), fin(hl).max(axis=1)) + np.abs(A0).sum(axis=1).max() * np.abs(x).max(axis=1)
    ineq = np.arange(m) >= meq
    lmin = np.where(act & ineq, np.abs(lam), np.inf).min(axis=1)
    smin = np.where(~act & ineq, slack, np.inf).min(axis=1)
    return (lmin > RF.STRICT * ln) & (smin > RF.STRICT * sc)


def _same(a, b, keys=RF.OUT):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in keys)


def _stat(H0, f, A0, x, lam):
    r = x @ H0.T + f + lam @ A0
    scale = 1.0 + np.abs(f).max(axis=1) + np.abs(H0).sum(axis=1).max() * np.abs(x).max(axis=1)
    return float((np.abs(r).max(axis=1) / scale).max())


# ------------------------------------------------------------------------ parity
@pytest.mark.parametrize("n,m,meq", RF.ROW_SHAPES)
def test_parity_with_the_unfactored_path_and_the_oracle(qpb, n, m, meq):
    for Bq in RF.BATCHES:
        H0, f, A0, bl, bu, _ = RF.family(Bq, n, m, meq)
        xr, lr, ar, wr, strict, ost = RF.oracle(Bq, n, m, meq)
        assert (ost == 0).all() and strict.mean() >= RF.MIN_STRICT_SHARE, (Bq, strict.mean())
        got, ref, fstatus = _both(qpb, H0, f, A0, bl, bu, meq)
        diff = np.abs(got["x"] - ref["x"]).max(axis=1) / (1.0 + np.abs(ref["x"]).max(axis=1))
        worst = RF.kkt(H0, f, A0, bl, bu, meq, got["x"], got["lam"])
        act, low = _masks(got, m)
        print(f"({n},{m},{meq}) B={Bq}: status {np.bincount(got['status'], minlength=5).tolist()} "
              f"x err {FC.relx(got['x'], xr).max():.2e} lam err {FC.rell(got['lam'], lr).max():.2e} "
              f"kkt {max(worst.values()):.2e} strict {int(strict.sum())}/{Bq} "
              f"upper {int((act & ~low)[:, meq:].sum())} lower {int(low.sum())} "
              f"iters differ {int((got['iters'] != ref['iters']).sum())} "
              f"factored vs unfactored x: worst relative difference {diff.max():.3e}")
        assert fstatus == OK
        assert np.array_equal(got["status"], ref["status"]) and (got["status"] == OK).all(), (Bq, got["status"])
        assert FC.relx(got["x"], xr).max() <= RF.X_TOL, Bq
        assert FC.rell(got["lam"], lr).max() <= RF.LAM_TOL, Bq
        assert all(v <= RF.KKT_TOL for v in worst.values()), (Bq, worst)
        assert np.array_equal(got["active"][strict], ref["active"][strict]), Bq
        assert np.array_equal(got["lower"][strict], ref["lower"][strict]), Bq
        assert np.array_equal(act[strict], ar[strict]) and np.array_equal(low[strict], wr[strict]), Bq
        assert act[:, :meq].all()
        _signs_agree(got["lam"], act, low, meq)


# --------------------------------------------------------------- status contract
def _contract(qpb, H0, f, A0, bl, bu, meq, max_iter=0):
    got, ref, fstatus = _both(qpb, H0, f, A0, bl, bu, meq, max_iter=max_iter)
    assert np.array_equal(got["status"], ref["status"]), (got["status"], ref["status"])
    return got, ref, fstatus


def _zeroed(got, rows):
    """What qpb.h promises for a failure found in the set-up."""
    assert (got["iters"][rows] == 0).all() and (got["lam"][rows] == 0).all()
    assert (got["active"][rows] == 0).all() and (got["lower"][rows] == 0).all()


@pytest.mark.parametrize("n,m,meq", CONTRACT_SHAPES)
def test_status_contract(qpb, n, m, meq):
    H0, f, A0, bl, bu, _ = RF.family(B, n, m, meq)
    xr, _, ar, wr, _, _ = RF.oracle(B, n, m, meq)
    every = np.arange(B)
    r = meq + 1  # an inequality row
    # an indefinite H: every QP NOT_SPD, and the factor says so
    Hn = H0.copy()
    Hn[n // 2, n // 2] = -1.0
    got, _, fstatus = _contract(qpb, Hn, f, A0, bl, bu, meq)
    assert fstatus == NOT_SPD and (got["status"] == NOT_SPD).all()
    _zeroed(got, every)
    # a NaN in one row of A: every QP NUMERICAL (found in the set-up)
    An = A0.copy()
    An[m - 3, 1] = np.nan
    got, _, fstatus = _contract(qpb, H0, f, An, bl, bu, meq)
    assert fstatus == NUMERICAL and (got["status"] == NUMERICAL).all()
    _zeroed(got, every)
    # a zero row of A is judged against each QP's own bounds: 0 above bu in some QPs, below bl in others
    Az, blz, buz = A0.copy(), bl.copy(), bu.copy()
    Az[m - 1] = 0.0
    blz[:, m - 1], buz[:, m - 1] = -1.0, 2.0
    blz[::3, m - 1], buz[::3, m - 1] = -2.0, -1.0
    blz[1::3, m - 1], buz[1::3, m - 1] = 1.0, 2.0
    got, ref, fstatus = _contract(qpb, H0, f, Az, blz, buz, meq)
    bad = np.zeros(B, bool)
    bad[::3] = bad[1::3] = True
    assert fstatus == OK and (got["status"][bad] == INFEASIBLE).all() and (got["status"][~bad] == OK).all()
    _zeroed(got, bad)
    assert FC.relx(got["x"][~bad], ref["x"][~bad]).max() <= RF.X_TOL
    x0 = np.linalg.solve(H0, -f.T).T
    assert np.allclose(got["x"][bad], x0[bad], rtol=1e-9, atol=1e-9)
    # bounds crossed beyond the threshold in some QPs only: INFEASIBLE from the set-up
    blc = bl.copy()
    blc[::4, r] = bu[::4, r] + 1e-3
    got, ref, _ = _contract(qpb, H0, f, A0, blc, bu, meq)
    bad = np.zeros(B, bool)
    bad[::4] = True
    assert (got["status"][bad] == INFEASIBLE).all() and (got["status"][~bad] == OK).all()
    _zeroed(got, bad)
    assert FC.relx(got["x"][~bad], ref["x"][~bad]).max() <= RF.X_TOL
    # a negative width inside the threshold, on a row the solution holds at its upper bound
    bln = bl.copy()
    hit = []
    for k in range(0, B, 5):
        rows = np.flatnonzero(ar[k] & ~wr[k] & (np.arange(m) >= meq))
        if len(rows):
            bln[k, rows[0]] = bu[k, rows[0]] + 0.5 * TOL * (np.linalg.norm(A0[rows[0]]) + abs(bu[k, rows[0]]))
            hit.append(k)
    assert len(hit) >= 3
    got, ref, _ = _contract(qpb, H0, f, A0, bln, bu, meq)
    assert (got["status"] == OK).all()
    assert FC.relx(got["x"], ref["x"]).max() <= RF.X_TOL and FC.relx(got["x"], xr).max() <= RF.X_TOL
    # a non-finite bu on an equality: NUMERICAL from the set-up, in those QPs only
    for value in (np.nan, np.inf, -np.inf):
        bue = bu.copy()
        bue[2::7, 0] = value
        bue[3::7, 1] = value
        got, _, _ = _contract(qpb, H0, f, A0, bl, bue, meq)
        bad = np.zeros(B, bool)
        bad[2::7] = bad[3::7] = True
        assert (got["status"][bad] == NUMERICAL).all() and (got["status"][~bad] == OK).all(), value
        _zeroed(got, bad)
    # a small max_iter: MAX_ITER with iters == max_iter and x = -H^-1 (f + A^T lam) for the signed lam
    for mi in (1, 2, meq + 3):
        got, _, _ = _contract(qpb, H0, f, A0, bl, bu, meq, max_iter=mi)
        capped = got["status"] == MAX_ITER
        assert capped.any() and (got["iters"][capped] == mi).all() and (got["status"][~capped] == OK).all()
        act, low = _masks(got, m)
        assert np.isfinite(got["x"]).all() and np.isfinite(got["lam"]).all()
        _signs_agree(got["lam"], act, low, meq)
        assert _stat(H0, f, A0, got["x"], got["lam"]) <= RF.KKT_TOL


# ------------------------------------------------------------------------- sides
@pytest.mark.parametrize("n,m,meq", CONTRACT_SHAPES)
def test_one_side_absent_everywhere(qpb, n, m, meq):
    H0, f, A0, bl, bu, _ = RF.family(B, n, m, meq)
    F = FC.factor(qpb, H0, A0)
    ineq = np.arange(m) >= meq
    # bu = None: every row >= meq is held lower-oriented from the load (the buffer's row of D negated).
    # An equality needs its bu, so this case has none: meq = 0 on the same rows.
    got = RF.solve(qpb, F, f, bl, None, 0)
    ref = RF.unfactored(qpb, H0, f, A0, bl, None, 0)
    act, low = _masks(got, m)
    assert np.array_equal(got["status"], ref["status"]) and (got["status"] == OK).all()
    assert FC.relx(got["x"], ref["x"]).max() <= RF.X_TOL and FC.rell(got["lam"], ref["lam"]).max() <= RF.LAM_TOL
    worst = RF.kkt(H0, f, A0, bl, np.full_like(bl, np.inf), 0, got["x"], got["lam"])
    assert all(v <= RF.KKT_TOL for v in worst.values()), worst
    assert np.array_equal(low, act) and act.any() and (got["lam"] <= 0).all()
    strict = _strict(A0, bl, None, 0, ref["x"], ref["lam"], RO.unpack_bits(ref["active"], m))
    assert strict.mean() >= RF.MIN_STRICT_SHARE
    assert np.array_equal(got["active"][strict], ref["active"][strict])
    # ... the same rows said with -inf in bu, bit for bit
    assert _same(RF.solve(qpb, F, f, bl, np.full_like(bu, np.inf), 0), got)
    # with the equalities: the lower bounds of the rows >= meq alone (bu finite on the equalities only)
    buo = bu.copy()
    buo[:, meq:] = np.inf
    got = RF.solve(qpb, F, f, bl, buo, meq)
    ref = RF.unfactored(qpb, H0, f, A0, bl, buo, meq)
    act, low = _masks(got, m)
    assert np.array_equal(got["status"], ref["status"]) and (got["status"] == OK).all()
    assert FC.relx(got["x"], ref["x"]).max() <= RF.X_TOL
    assert np.array_equal(low[:, ineq], act[:, ineq]) and not low[:, ~ineq].any() and act[:, ~ineq].all()
    _signs_agree(got["lam"], act, low, meq)
    # bl = None: the one-sided problem -- the same x and the same active as qpb_solve_factored on (A, bu)
    one = FC.solve(qpb, F, f, bu, meq)
    got = RF.solve(qpb, F, f, None, bu, meq)
    assert np.array_equal(got["status"], one["status"]) and (got["status"] == OK).all()
    rel = np.abs(got["x"] - one["x"]).max(axis=1) / np.maximum(1.0, np.abs(one["x"]).max(axis=1))
    assert rel.max() <= 1e-9, rel.max()
    assert np.array_equal(got["active"], one["active"]) and not got["lower"].any()
    assert (got["lam"][:, meq:] >= 0).all()
    assert _same(RF.solve(qpb, F, f, np.full_like(bl, -np.inf), bu, meq), got)


@pytest.mark.parametrize("n,m,meq", CONTRACT_SHAPES)
def test_absent_sides_in_single_entries(qpb, n, m, meq):
    H0, f, A0, bl, bu, _ = RF.family(B, n, m, meq)
    r = meq + 1
    bl2, bu2 = bl.copy(), bu.copy()
    bu2[1::6, r] = np.nan            # the upper side absent
    bu2[2::6, r] = -np.inf           # ... -inf is absent too, not "never satisfiable"
    bl2[3::6, r + 1] = np.inf        # the lower side absent
    bl2[4::6, r + 1] = np.nan
    bl2[5::6, r + 2] = -np.inf       # absent on both sides: the row does not exist
    bu2[5::6, r + 2] = np.nan
    got, ref, _ = _both(qpb, H0, f, A0, bl2, bu2, meq)
    act, low = _masks(got, m)
    assert np.array_equal(got["status"], ref["status"]) and (got["status"] == OK).all()
    assert FC.relx(got["x"], ref["x"]).max() <= RF.X_TOL and FC.rell(got["lam"], ref["lam"]).max() <= RF.LAM_TOL
    worst = RF.kkt(H0, f, A0, bl2, bu2, meq, got["x"], got["lam"])
    assert all(v <= RF.KKT_TOL for v in worst.values()), worst
    _signs_agree(got["lam"], act, low, meq)
    # a row is never active on a side it does not have
    for k0 in (1, 2):
        assert np.array_equal(act[k0::6, r], low[k0::6, r])
    for k0 in (3, 4):
        assert not low[k0::6, r + 1].any()
    assert not act[5::6, r + 2].any()
    strict = _strict(A0, bl2, bu2, meq, ref["x"], ref["lam"], RO.unpack_bits(ref["active"], m))
    assert strict.mean() >= RF.MIN_STRICT_SHARE
    assert np.array_equal(got["active"][strict], ref["active"][strict])
    assert np.array_equal(got["lower"][strict], ref["lower"][strict])


@pytest.mark.parametrize("n,m,meq", CONTRACT_SHAPES)
def test_zero_width_row(qpb, n, m, meq):
    """bl = bu on a row >= meq: the x of the form that says the row with meq."""
    H0, f, A0, bl, bu, _ = RF.family(B, n, m, meq)
    xr, _, ar, wr, _, _ = RF.oracle(B, n, m, meq)
    # A is shared, so the pinned row is the same one in every QP: the row >= meq
    # that most solutions hold active, swapped to index meq (so that the same
    # row can be said with meq + 1), pinned at the bound it sits at in the QPs
    # whose solution x* holds it active (x* stays the solution); the other QPs
    # are left out
    r = meq + int(ar[:, meq:].sum(axis=0).argmax())
    pin = ar[:, r]
    assert pin.sum() >= 5 and wr[pin, r].any() and not wr[pin, r].all()  # taken from either side
    A2, bl2, bu2 = A0.copy(), bl[pin].copy(), bu[pin].copy()
    bl2[:, r] = bu2[:, r] = np.where(wr[pin, r], bl[pin, r], bu[pin, r])
    A2[[meq, r]] = A2[[r, meq]]
    bl2[:, [meq, r]] = bl2[:, [r, meq]]
    bu2[:, [meq, r]] = bu2[:, [r, meq]]
    F = FC.factor(qpb, H0, A2)
    got = RF.solve(qpb, F, f[pin], bl2, bu2, meq)
    want = RF.solve(qpb, F, f[pin], bl2, bu2, meq + 1)  # row meq as an equality a x = bu
    assert (got["status"] == OK).all() and (want["status"] == OK).all()
    assert FC.relx(got["x"], want["x"]).max() <= RF.X_TOL and FC.relx(got["x"], xr[pin]).max() <= RF.X_TOL
    worst = RF.kkt(H0, f[pin], A2, bl2, bu2, meq, got["x"], got["lam"])
    assert all(v <= RF.KKT_TOL for v in worst.values()), worst
    act, low = _masks(got, m)
    assert act[:, meq].all()
    assert low[:, meq].any() and not low[:, meq].all()


@pytest.mark.parametrize("n,m,meq", CONTRACT_SHAPES)
def test_rows_active_opposite_to_their_first_violation(qpb, n, m, meq):
    """range_oracle.side_counts' "opposite" rows on this family: violated on one
    side at the unconstrained minimum, active on the other at the solution, so
    the row of D loaded from the buffer is re-oriented in place during the loop."""
    H0, f, A0, bl, bu, _ = RF.family(B, n, m, meq)
    xr, _, ar, wr, strict, _ = RF.oracle(B, n, m, meq)
    a0 = np.linalg.solve(H0, -f.T).T @ A0.T
    ineq = np.arange(m) >= meq
    opp = ((ar & wr & (a0 > bu)) | (ar & ~wr & (a0 < bl))) & ineq
    has = opp.any(axis=1) & strict
    assert has.sum() >= 5
    got = RF.solve(qpb, FC.factor(qpb, H0, A0), f[has], bl[has], bu[has], meq)
    act, low = _masks(got, m)
    assert (got["status"] == OK).all() and FC.relx(got["x"], xr[has]).max() <= RF.X_TOL
    assert np.array_equal(act, ar[has]) and np.array_equal(low, wr[has])
    assert (got["iters"] > act.sum(axis=1)).all()


# ---------------------------------------------------------------------- plumbing
@pytest.mark.parametrize("n,m,meq", [(5, 9, 2), (16, 32, 4), (16, 16, 3), (20, 40, 4)])
def test_lower_null_and_iters_null_change_nothing(qpb, n, m, meq):
    Bq = 5
    H0, f, A0, bl, bu, _ = RF.family(Bq, n, m, meq)
    F = FC.factor(qpb, H0, A0)
    a = RF.solve(qpb, F, f, bl, bu, meq)
    for kw in ({"iters": False}, {"lower": False}, {"iters": False, "lower": False}):
        c = RF.solve(qpb, F, f, bl, bu, meq, **kw)
        assert not any(k in c for k in kw)
        assert _same(a, c, keys=list(c))


def _bits(a, k):
    """QP k's part of an output, as bytes."""
    return np.ascontiguousarray(a[k:k + 1]).tobytes()


@pytest.mark.parametrize("n,m,meq", RF.ROW_SHAPES)
def test_outputs_do_not_depend_on_batch_or_slot(qpb, n, m, meq):
    """QP k bitwise the same alone (B = 1) and in its place in B = 67: every slot
    of a full group of four, and the ragged last group's live rows."""
    H0, f, A0, bl, bu, _ = RF.family(B, n, m, meq)
    F = FC.factor(qpb, H0, A0)
    big = RF.solve(qpb, F, f, bl, bu, meq)
    for k in (0, 1, 2, 3, 64, 65, 66):
        one = RF.solve(qpb, F, f[k:k + 1], bl[k:k + 1], bu[k:k + 1], meq)
        for key in RF.OUT:
            assert _bits(one[key], 0) == _bits(big[key], k), (k, key)
    five = RF.solve(qpb, F, f[2:7], bl[2:7], bu[2:7], meq)  # ... and at another slot of another batch
    assert all(_bits(five[key], 3) == _bits(big[key], 5) for key in RF.OUT)


@pytest.mark.parametrize("n,m,meq", CONTRACT_SHAPES + [(16, 16, 3)])
def test_one_buffer_serves_both_solves_and_is_not_written(qpb, n, m, meq):
    H0, f, A0, bl, bu, _ = RF.family(B, n, m, meq)
    F = FC.factor(qpb, H0, A0)
    before = FC.factor_result(F)[0].copy()
    one_sided = FC.solve(qpb, F, f, bu, meq)
    first = RF.solve(qpb, F, f, bl, bu, meq)
    one_sided_again = FC.solve(qpb, F, f, bu, meq)
    again = RF.solve(qpb, F, f, bl, bu, meq)
    assert np.array_equal(FC.factor_result(F)[0].view(np.uint8), before.view(np.uint8)), "a solve wrote to fac"
    assert _same(first, again)
    assert all(np.array_equal(one_sided[k].view(np.uint8), one_sided_again[k].view(np.uint8)) for k in FC.OUT)
    assert (first["status"] == OK).all() and (one_sided["status"] == OK).all()
    assert FC.relx(first["x"], RF.oracle(B, n, m, meq)[0]).max() <= RF.X_TOL
    assert FC.relx(one_sided["x"], FC.oracle(B, n, m, meq)[0]).max() <= FC.X_TOL


@pytest.mark.parametrize("n,m,meq", CONTRACT_SHAPES)
def test_factor_then_solve_on_a_side_stream_without_host_sync(qpb, n, m, meq):
    H0, f, A0, bl, bu, _ = RF.family(B, n, m, meq)
    ref = RF.solve(qpb, FC.factor(qpb, H0, A0), f, bl, bu, meq)
    side = torch.cuda.Stream()
    fd, bld, bud = FC.dev(f), FC.dev(bl), FC.dev(bu)  # uploaded first: nothing below waits on the host
    torch.cuda.synchronize()
    F = FC.factor(qpb, H0, A0, stream=side, sync=False)
    got = RF.solve(qpb, F, fd, bld, bud, meq, stream=side)
    assert _same(got, ref)
    assert FC.factor_result(F)[1] == OK


@pytest.mark.parametrize("n", [3, 16, 20])
def test_no_rows_is_qpb_solve_factored(qpb, n):
    """m == 0: the outputs of qpb_solve_factored bit for bit, and `lower` is not written."""
    for Bq in (1, 5, 67):
        H0, f, A0, _ = SC.family(Bq, n, 0, 0)
        F = FC.factor(qpb, H0, A0)
        want = FC.solve(qpb, F, f, None, 0)
        got = RF.solve(qpb, F, f, None, None, 0)
        assert all(np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)) for k in FC.OUT)
        assert (got["status"] == OK).all()
        assert _stat(H0, f, np.zeros((0, n)), got["x"], got["lam"]) <= RF.KKT_TOL
    # a `lower` pointer given at m == 0 is left alone
    d = qpb.Desc(n, 0, Bq, 0, 0, 0.0)
    low = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    x = torch.empty((Bq, n), dtype=torch.float64, device="cuda")
    st = torch.empty((Bq,), dtype=torch.int32, device="cuda")
    import ctypes
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = qpb.lib().qpb_solve_range_factored(ctypes.byref(d), 0, p(F[0][F[1]:]), p(FC.dev(f)), None, None, p(x), None,
                                            None, p(low), p(st), None, None)
    torch.cuda.synchronize()
    assert rc == 0 and (low.cpu().numpy() == 0x5A5A5A5A).all()
    assert np.array_equal(x.cpu().numpy().view(np.uint8), want["x"].view(np.uint8))


# ------------------------------------------------------------------- the binding
def test_python_binding(qpb):
    n, m, meq, Bq = 16, 32, 4, 5
    H0, f, A0, bl, bu, _ = RF.family(Bq, n, m, meq)
    F = qpb.factor_shared(FC.dev(H0), FC.dev(A0))
    sol = qpb.solve_range_factored(F, FC.dev(f), FC.dev(bl), FC.dev(bu), meq)
    torch.cuda.synchronize()
    ref = RF.solve(qpb, FC.factor(qpb, H0, A0), f, bl, bu, meq)
    assert isinstance(sol, qpb.RangeSolution) and int(F.status.item()) == OK
    for k in RF.OUT:
        assert np.array_equal(getattr(sol, k).cpu().numpy().view(np.uint8), ref[k].view(np.uint8)), k
    # either bound may be None
    up = qpb.solve_range_factored(F, FC.dev(f), None, FC.dev(bu), meq)
    torch.cuda.synchronize()
    assert np.array_equal(up.x.cpu().numpy(), RF.solve(qpb, FC.factor(qpb, H0, A0), f, None, bu, meq)["x"])
    # the host form: the same bits
    Fh = qpb.factor_shared_host(H0, A0)
    hs = qpb.solve_range_factored_host(Fh, f, bl, bu, meq)
    for k in RF.OUT:
        assert np.array_equal(np.asarray(getattr(hs, k)).view(np.uint8), ref[k].view(np.uint8)), k
    # shapes that do not match the factor's (n, m)
    with pytest.raises(ValueError):
        qpb.solve_range_factored(F, FC.dev(f[:, :5].copy()), FC.dev(bl), FC.dev(bu), meq)
    with pytest.raises(ValueError):
        qpb.solve_range_factored(F, FC.dev(f), FC.dev(bl[:, :9].copy()), FC.dev(bu), meq)
    with pytest.raises(ValueError):
        qpb.solve_range_factored(F, FC.dev(f), FC.dev(bl), FC.dev(bu[:3].copy()), meq)
    with pytest.raises(ValueError):
        qpb.solve_range_factored(F, FC.dev(f), None, None, meq)
    with pytest.raises(ValueError):
        qpb.solve_range_factored(qpb.SharedFactor(F.fac, 20, 40, F.status), FC.dev(np.zeros((Bq, 20))),
                                 FC.dev(np.zeros((Bq, 40))), FC.dev(np.ones((Bq, 40))))
