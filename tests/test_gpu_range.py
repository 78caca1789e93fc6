"""qpb_solve_range on the GPU: two-sided rows bl <= A x <= bu in the RG forms
of the two wavefront-level kernels (gi_dense: n <= 16, m <= 32, four QPs per
wavefront; gi_wave: n <= 32, m <= 64).

The reference is tests/range_oracle.py (the pair rewrite [E; G; -G] through
eq_oracle.eq_solve, mapped back) and its two-sided KKT certificate.  Bars are
the project's: x and lambda within 1e-6 relative, `active` and `lower`
bit-exact, certificate <= 1e-9.  "Bitwise" compares two launches on the same
QP.  The batch of 67 leaves the four-per-wave kernel a ragged last wave.
iters counts loop trips as in test_gpu_eq.py: `iters > set bits + 1` shows a
DROP.
"""
import numpy as np
import pytest

import range_oracle as RO

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

X_TOL = 1e-6
KKT_TOL = 1e-9
OK, MAX_ITER, NOT_SPD, INFEASIBLE, NUMERICAL = 0, 1, 2, 3, 4
B = 67

# (n, m, meq)
DENSE_SHAPES = [(16, 32, 0), (16, 32, 4), (16, 16, 3), (7, 13, 3), (1, 2, 0)]
WAVE_SHAPES = [(16, 33, 5), (20, 33, 5), (32, 64, 8)]
CLASSES = [(16, 32, 4), (20, 33, 5)]  # one shape of each kernel class


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    return q


def _dev(*arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
            for a in arrays]


def _host(sol):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in sol]


FILL8 = np.frombuffer(bytes([0xA5] * 8), dtype=np.int64)[0]
FILL4 = np.frombuffer(bytes([0xA5] * 4), dtype=np.int32)[0]
NAMES = ("x", "lam", "active", "lower", "status", "iters")


def _solve_range(qpb, H, f, A, bl, bu, meq=0, **kw):
    """solve_range into outputs filled with 0xA5: every element of every
    output, `lower` included, must have been written, whatever the status."""
    Bq, n = f.shape
    m = A.shape[-2]
    out = qpb._empty_range_solution(Bq, n, m, torch.device("cuda"))
    for t in out:
        t.view(torch.uint8).fill_(0xA5)
    sol = _host(qpb.solve_range(*_dev(H, f, A, bl, bu), meq, out=out, **kw))
    for name, a in zip(NAMES, sol):
        raw = a.view(np.int64) if a.dtype == np.float64 else a.view(np.int32)
        assert not (raw == (FILL8 if a.dtype == np.float64 else FILL4)).any(), (name, "elements never written")
    return sol


def _solve_eq(qpb, H, f, A, b, meq, **kw):
    return _host(qpb.solve_eq(*_dev(H, f, A, b), meq, **kw))


def _same(a, b):
    return all(np.array_equal(u.view(np.uint8), v.view(np.uint8)) for u, v in zip(a, b))


def _take(sol, idx):
    return [v[idx] for v in sol]


def _relx(x, xr):
    return np.abs(x - xr).max(axis=1) / np.maximum(1.0, np.abs(xr).max(axis=1))


def _rell(lam, lr):
    return np.abs(lam - lr).max(axis=1) / (1.0 + np.abs(lr).max(axis=1))


def _signs_agree(lam, act, low, meq):
    """lam is 0 outside active; on the rows >= meq a nonzero lam is negative
    exactly where the lower bit is set; lower is a subset of active and clear
    on the equalities."""
    assert not (low & ~act).any()
    assert not low[:, :meq].any()
    assert (lam[~act] == 0).all()
    li, lo = lam[:, meq:], low[:, meq:]
    nz = li != 0
    assert np.array_equal((li < 0)[nz], lo[nz])


def _stationarity(H, f, A, x, lam):
    r = np.einsum("bij,bj->bi", H, x) + f + np.einsum("bij,bi->bj", A, lam)
    sc = 1.0 + np.abs(f).max(axis=1) + np.abs(H).sum(axis=2).max(axis=1) * np.abs(x).max(axis=1)
    return (np.abs(r).max(axis=1) / sc).max()


# ---------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("n,m,meq", DENSE_SHAPES + WAVE_SHAPES)
def test_parity(qpb, n, m, meq):
    H, f, A, bl, bu, xc, refs = RO.range_reference(B, n, m, meq)
    x, lam, act, low, st, it = _solve_range(qpb, H, f, A, bl, bu, meq)
    mask, lmask = RO.unpack_bits(act, m), RO.unpack_bits(low, m)
    xr = np.array([r.x for r in refs])
    lr = np.array([r.lam for r in refs])
    ar = np.array([r.active for r in refs])
    wr = np.array([r.lower for r in refs])
    worst = {k: float(v.max()) for k, v in RO.kkt_range(H, f, A, bl, bu, meq, x, lam).items()}
    bits = mask.sum(axis=1)
    drops = int((it > bits + 1).sum())
    print(f"({n},{m},{meq}): status {np.bincount(st, minlength=5).tolist()} x err {_relx(x, xr).max():.2e} "
          f"lam err {_rell(lam, lr).max():.2e} kkt {max(worst.values()):.2e} "
          f"active mismatches {int((mask != ar).any(axis=1).sum())} lower mismatches "
          f"{int((lmask != wr).any(axis=1).sum())} iters {it.min()}..{it.max()} QPs with a DROP {drops} "
          f"upper {int((mask & ~lmask)[:, meq:].sum())} lower {int(lmask.sum())}")
    assert (st == OK).all(), st
    assert _relx(x, xr).max() <= X_TOL
    assert _rell(lam, lr).max() <= 1e-6
    assert np.array_equal(mask, ar)
    assert np.array_equal(lmask, wr)
    assert all(v <= KKT_TOL for v in worst.values()), worst
    _signs_agree(lam, mask, lmask, meq)
    assert (it > bits).all() and (it <= 4 * (n + m) + 8).all()
    if n - meq >= 2:
        assert drops >= 1
        assert lmask.any() and (mask & ~lmask)[:, meq:].any()  # both sides are exercised


# ------------------------------------------------- 2. the pair rewrite on the GPU
@pytest.mark.parametrize("n,m,meq", [(16, 32, 0), (16, 16, 3), (7, 13, 3), (16, 33, 5), (1, 2, 0)])
def test_pair_rewrite(qpb, n, m, meq):
    assert 2 * m - meq <= 64
    H, f, A, bl, bu, _, _ = RO.range_reference(B, n, m, meq)
    x, lam, act, low, st, it = _solve_range(qpb, H, f, A, bl, bu, meq)
    A2, b2 = RO.to_pairs(A, bl, bu, meq)
    x2, lam2, act2, st2, it2 = _solve_eq(qpb, H, f, A2, b2, meq)
    assert (st == OK).all() and (st2 == OK).all()
    mask2 = RO.unpack_bits(act2, 2 * m - meq)
    k = m - meq
    both = np.concatenate([mask2[:, :meq], mask2[:, meq:meq + k] | mask2[:, meq + k:]], axis=1)
    print(f"({n},{m},{meq}): x diff {_relx(x, x2).max():.2e}; iters {it.mean():.2f} range, {it2.mean():.2f} pairs")
    assert _relx(x, x2).max() <= X_TOL
    assert np.array_equal(RO.unpack_bits(act, m), both)
    assert np.array_equal(RO.unpack_bits(low, m)[:, meq:], mask2[:, meq + k:])


# ---------------------------------------------------------------------- 3. mirror
@pytest.mark.parametrize("n,m,meq", [(16, 32, 4), (7, 13, 3), (20, 33, 5)])
def test_mirror(qpb, n, m, meq):
    H, f, A, bl, bu, _, _ = RO.range_reference(B, n, m, meq)
    x, lam, act, low, st, _ = _solve_range(qpb, H, f, A, bl, bu, meq)
    Am, blm, bum = A.copy(), bl.copy(), bu.copy()
    Am[:, meq:] = -A[:, meq:]
    blm[:, meq:] = -bu[:, meq:]
    bum[:, meq:] = -bl[:, meq:]
    xm, lamm, actm, lowm, stm, _ = _solve_range(qpb, H, f, Am, blm, bum, meq)
    assert (st == OK).all() and (stm == OK).all()
    assert _relx(xm, x).max() <= X_TOL
    want = lam.copy()
    want[:, meq:] = -lam[:, meq:]
    assert _rell(lamm, want).max() <= 1e-6
    mask, lmask = RO.unpack_bits(act, m), RO.unpack_bits(low, m)
    assert np.array_equal(RO.unpack_bits(actm, m), mask)
    assert np.array_equal(RO.unpack_bits(lowm, m)[:, meq:], (mask & ~lmask)[:, meq:])
    assert not RO.unpack_bits(lowm, m)[:, :meq].any()


# ------------------------------------------------------------------- 4. one-sided
@pytest.mark.parametrize("n,m,meq", [(16, 32, 4), (7, 13, 3), (20, 33, 5)])
def test_one_sided(qpb, n, m, meq):
    H, f, A, bl, bu, _, _ = RO.range_reference(B, n, m, meq)
    want = _solve_eq(qpb, H, f, A, bu, meq)
    assert (want[3] == OK).all()
    a = _solve_range(qpb, H, f, A, np.full_like(bl, -np.inf), bu, meq)
    b = _solve_range(qpb, H, f, A, None, bu, meq)
    assert _same(a, b)
    x, lam, act, low, st, it = a
    print(f"({n},{m},{meq}) upper only: {int((it != want[4]).sum())} of {B} QPs differ in iters from solve_eq")
    assert np.array_equal(st, want[3]) and np.array_equal(act, want[2]) and not low.any()
    assert _relx(x, want[0]).max() <= X_TOL and _rell(lam, want[1]).max() <= 1e-6
    # the lower bounds alone: the pre-orientation path, against solve_eq on (-A, -bl)
    An, bn = A.copy(), bu.copy()
    An[:, meq:] = -A[:, meq:]
    bn[:, meq:] = -bl[:, meq:]
    want = _solve_eq(qpb, H, f, An, bn, meq)
    assert (want[3] == OK).all()
    buo = bu.copy()
    buo[:, meq:] = np.inf
    x, lam, act, low, st, it = _solve_range(qpb, H, f, A, bl, buo, meq)
    print(f"({n},{m},{meq}) lower only: {int((it != want[4]).sum())} of {B} QPs differ in iters from solve_eq")
    assert np.array_equal(st, want[3]) and np.array_equal(act, want[2])
    mask = RO.unpack_bits(act, m)
    assert np.array_equal(RO.unpack_bits(low, m)[:, meq:], mask[:, meq:]) and not RO.unpack_bits(low, m)[:, :meq].any()
    wl = want[1].copy()
    wl[:, meq:] = -wl[:, meq:]
    assert _relx(x, want[0]).max() <= X_TOL and _rell(lam, wl).max() <= 1e-6


# ------------------------------------------------------------------- 5. zero width
@pytest.mark.parametrize("n,m,meq", [(16, 32, 4), (20, 33, 5)])
def test_zero_width(qpb, n, m, meq):
    H, f, A, bl, bu, _, refs = RO.range_reference(B, n, m, meq)
    # Two rows of every QP that its solution holds active, one side or the
    # other, get bl = bu = the bound they sit at, and are swapped to the rows
    # meq, meq + 1: pinned there the QP stays feasible (a row pinned anywhere
    # else may empty the feasible set), and the same rows can be said with meq.
    A, bl, bu = A.copy(), bl.copy(), bu.copy()
    for i, r in enumerate(refs):
        rows = np.flatnonzero(r.active & (np.arange(m) >= meq))[:2]
        assert len(rows) == 2, i
        for dst, src in zip((meq, meq + 1), rows):
            v = bl[i, src] if r.lower[src] else bu[i, src]
            bl[i, src] = bu[i, src] = v
            for arr in (A, bl, bu):
                arr[i, [dst, src]] = arr[i, [src, dst]]
    assert np.array_equal(bl[:, meq:meq + 2], bu[:, meq:meq + 2])
    want = _solve_range(qpb, H, f, A, bl, bu, meq + 2)  # rows meq, meq + 1 as equalities a x = bu
    x, lam, act, low, st, it = _solve_range(qpb, H, f, A, bl, bu, meq)
    assert (st == OK).all() and (want[4] == OK).all()
    assert _relx(x, want[0]).max() <= X_TOL
    assert _relx(x, np.array([r.x for r in refs])).max() <= X_TOL
    cert = RO.kkt_range(H, f, A, bl, bu, meq, x, lam)
    assert max(v.max() for v in cert.values()) <= KKT_TOL
    mask, lmask = RO.unpack_bits(act, m), RO.unpack_bits(low, m)
    assert mask[:, meq:meq + 2].all()
    assert lmask[:, meq:meq + 2].any() and not lmask[:, meq:meq + 2].all()  # taken from either side


# ----------------------------------------------------------------------- 6. shared
@pytest.mark.parametrize("n,m,meq", CLASSES)
def test_shared(qpb, n, m, meq):
    H, f, A, bl, bu, xc, _ = RO.range_reference(B, n, m, meq)
    # one H and one A: bounds around every QP's own point keep the batch feasible
    H0, A0 = H[0], A[0]
    ax = np.einsum("ij,bj->bi", A0, xc)
    rng = np.random.default_rng([n, m, 5])
    buS = ax + rng.uniform(0.05, 1.0, size=ax.shape)
    blS = ax - rng.uniform(0.05, 1.0, size=ax.shape)
    blS[:, :meq] = buS[:, :meq] = ax[:, :meq]
    Hb, Ab = np.broadcast_to(H0, H.shape).copy(), np.broadcast_to(A0, A.shape).copy()
    want = _solve_range(qpb, Hb, f, Ab, blS, buS, meq)
    assert (want[4] == OK).all()
    assert RO.unpack_bits(want[3], m).any() and RO.unpack_bits(want[2], m).sum() > RO.unpack_bits(want[3], m).sum()
    for Hs, As in ((H0, Ab), (Hb, A0), (H0, A0)):
        assert _same(_solve_range(qpb, Hs, f, As, blS, buS, meq), want)


# ----------------------------------------------------------------- 7. independence
@pytest.mark.parametrize("n,m,meq", CLASSES)
def test_independence(qpb, n, m, meq):
    H, f, A, bl, bu, _, _ = RO.range_reference(B, n, m, meq)
    full = _solve_range(qpb, H, f, A, bl, bu, meq)
    for k in (0, 5, 66):
        one = _solve_range(qpb, H[k:k + 1], f[k:k + 1], A[k:k + 1], bl[k:k + 1], bu[k:k + 1], meq)
        assert _same(one, _take(full, slice(k, k + 1))), k
        idx = [1, 2, 3, 4, k]
        five = _solve_range(qpb, H[idx], f[idx], A[idx], bl[idx], bu[idx], meq)
        assert _same(_take(five, slice(4, 5)), _take(full, slice(k, k + 1))), k
    # a neighbour in the same wave with NaN inputs, and one with crossed bounds
    Hn, fn, bln, bun = H.copy(), f.copy(), bl.copy(), bu.copy()
    Hn[1] = np.nan
    fn[2] = np.nan
    bln[6, meq], bun[6, meq] = 5.0, -5.0
    got = _solve_range(qpb, Hn, fn, A, bln, bun, meq)
    keep = [k for k in range(B) if k not in (1, 2, 6)]
    assert _same(_take(got, keep), _take(full, keep))
    assert got[4][6] == INFEASIBLE and got[4][1] != OK and got[4][2] != OK


# --------------------------------------------------------------- 8. status contract
@pytest.mark.parametrize("n,m,meq", CLASSES)
def test_status_contract(qpb, n, m, meq):
    H, f, A, bl, bu, xc, refs = RO.range_reference(B, n, m, meq)
    K = 12
    H, f, A, bl, bu, xc = (v[:K].copy() for v in (H, f, A, bl, bu, xc))
    base = _solve_range(qpb, H, f, A, bl, bu, meq)
    assert (base[4] == OK).all()
    r = meq + 1  # an inequality row
    tol = 1e-10
    bl2, bu2, A2 = bl.copy(), bu.copy(), A.copy()
    # 0: crossed beyond the tolerance; 1: crossed inside it, on a row that is active
    # at its upper bound (so a x = bu is attainable)
    bl2[0, r] = bu[0, r] + 1e-3
    r1 = int(np.flatnonzero(refs[1].active & ~refs[1].lower & (np.arange(m) >= meq))[0])
    bl2[1, r1] = bu[1, r1] + 0.5 * tol * (np.linalg.norm(A[1, r1]) + abs(bu[1, r1]))
    # 2, 3: a zero row with 0 above bu / below bl; 4: a zero row with 0 inside
    A2[2:5, r] = 0.0
    bl2[2, r], bu2[2, r] = -2.0, -1.0
    bl2[3, r], bu2[3, r] = 1.0, 2.0
    bl2[4, r], bu2[4, r] = -1.0, 2.0
    # 5: NaN in bu only; 6: NaN in bl only; 7: both
    bu2[5, r] = np.nan
    bl2[6, r] = np.nan
    bl2[7, r] = bu2[7, r] = np.nan
    x, lam, act, low, st, it = got = _solve_range(qpb, H, f, A2, bl2, bu2, meq)
    mask, lmask = RO.unpack_bits(act, m), RO.unpack_bits(low, m)
    assert not (lmask & ~mask).any()
    for k in (0, 2, 3):
        assert st[k] == INFEASIBLE and it[k] == 0, (k, st[k], it[k])
        assert (lam[k] == 0).all() and not mask[k].any() and not lmask[k].any()
        assert np.allclose(x[k], np.linalg.solve(H[k], -f[k]), rtol=1e-9, atol=1e-9)
    assert st[1] == OK and st[4] == OK and (st[5:8] == OK).all()
    assert _same(_take(got, slice(8, K)), _take(base, slice(8, K)))
    # an absent side or row: the pair form with +inf there is the specification
    cert = RO.kkt_range(H[4:8], f[4:8], A2[4:8], bl2[4:8], bu2[4:8], meq, x[4:8], lam[4:8])
    assert max(v.max() for v in cert.values()) <= KKT_TOL
    assert not mask[4, r] and not mask[7, r] and not lmask[5, r] and not (mask[6, r] and lmask[6, r])
    for k, (lo_k, hi_k) in ((5, (bl[5], np.where(np.arange(m) == r, np.inf, bu[5]))),
                            (6, (np.where(np.arange(m) == r, -np.inf, bl[6]), bu[6])),
                            (7, (np.where(np.arange(m) == r, -np.inf, bl[7]), np.where(np.arange(m) == r, np.inf, bu[7])))):
        ref = RO.range_solve(H[k], f[k], A[k], lo_k, hi_k, meq, xc[k])
        assert ref.status == 0
        assert np.abs(x[k] - ref.x).max() <= X_TOL * max(1.0, np.abs(ref.x).max()), k
        assert np.array_equal(mask[k], ref.active) and np.array_equal(lmask[k], ref.lower), k
    # a non-finite bu on an equality
    if meq:
        for bad in (np.nan, np.inf, -np.inf):
            bu3 = bu.copy()
            bu3[3, 0] = bad
            got = _solve_range(qpb, H, f, A, bl, bu3, meq)
            assert got[4][3] == NUMERICAL, (bad, got[4][3])
            keep = [k for k in range(K) if k != 3]
            assert _same(_take(got, keep), _take(base, keep))
    # max_iter = 1, 2
    for mi in (1, 2):
        x, lam, act, low, st, it = _solve_range(qpb, H, f, A, bl, bu, meq, max_iter=mi)
        mask, lmask = RO.unpack_bits(act, m), RO.unpack_bits(low, m)
        assert (st == MAX_ITER).all() and (it == mi).all()
        assert np.isfinite(lam).all() and np.isfinite(x).all()
        _signs_agree(lam, mask, lmask, meq)
        assert _stationarity(H, f, A, x, lam) <= 1e-9
