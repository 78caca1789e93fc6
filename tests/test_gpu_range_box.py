"""qpb_solve_range_box on the GPU: two-sided rows beside variable bounds in the
BX forms of the range kernels (gi_dense: n <= 16, mg + n <= 32, four QPs per
wavefront; gi_wave: n <= 32, mg + n <= 64).

The specification is qpb_solve_range on the materialised [G; I], [bl; lb],
[bu; ub]: "bit for bit" compares the call with `qpb.solve_range` on those
tensors, torch.equal on all six outputs.  The oracle is tests/range_box_oracle.py
(range_oracle on the materialised problem); the bars are the project's: x and
lam within 1e-6 relative, `active` and `lower` bit-exact, certificate <= 1e-9.
The shapes cover the three load paths of gi_dense at one and two rows per lane
(FULL: (16,16) and (16,0); N16: (16,7), (16,1); padded: n < 16), general rows
that end inside a lane row ((12,20), (3,29), (7,9)), mg = 0, meq > 0, the class
edge (16,17) and the wave form padded and full.  Batches 1, 3, 5, 67 and 257
are the first QPs of one family of 257 per shape: 67 and 257 leave the
four-per-wave kernel a ragged last wave.
"""
import numpy as np
import pytest

import range_box_oracle as BO
import range_oracle as RO

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

X_TOL = 1e-6
KKT_TOL = 1e-9
OK, MAX_ITER, NOT_SPD, INFEASIBLE, NUMERICAL = 0, 1, 2, 3, 4
BATCHES = (1, 3, 5, 67, 257)
BMAX = max(BATCHES)
# one shape of every load path and class for the tests that perturb a batch
CLASSES = [(16, 16, 2), (16, 7, 0), (12, 20, 0), (16, 0, 0), (16, 17, 1), (20, 9, 0)]
NAMES = ("x", "lam", "active", "lower", "status", "iters")


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


def _box(qpb, H, f, G, bl, bu, lb, ub, meq=0, **kw):
    """solve_range_box on device copies; G with no rows is passed as None."""
    if G is not None and G.shape[-2] == 0:
        G = bl = bu = None
    return qpb.solve_range_box(*_dev(H, f, G, bl, bu, lb, ub), meq, **kw)


def _mat(qpb, H, f, G, bl, bu, lb, ub, meq=0, **kw):
    """The specification: solve_range on the materialised tensors.  H and G may
    be 2-D (one matrix for the batch): then A' = [G; I] is 2-D as well."""
    B, n = f.shape
    mg = 0 if G is None else G.shape[-2]
    if G is None:
        A = np.broadcast_to(np.eye(n), (B, n, n))
    elif G.ndim == 2:
        A = np.concatenate([G, np.eye(n)], axis=0)
    else:
        A = np.concatenate([G, np.broadcast_to(np.eye(n), (B, n, n))], axis=1)
    half = lambda v, k, fill: np.full((B, k), fill) if v is None else v  # noqa: E731
    lo = np.concatenate([half(bl, mg, -np.inf), half(lb, n, -np.inf)], axis=1)
    hi = np.concatenate([half(bu, mg, np.inf), half(ub, n, np.inf)], axis=1)
    return qpb.solve_range(*_dev(H, f, A, lo, hi), meq, **kw)


def _equal(a, b):
    torch.cuda.synchronize()
    # torch.equal on the bits: x and lam as 64-bit words, so that a failed QP's
    # NaN equals itself and -0.0 does not equal 0.0
    bits = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t  # noqa: E731
    bad = [name for name, u, v in zip(NAMES, a, b) if u.shape != v.shape or not torch.equal(bits(u), bits(v))]
    assert not bad, bad


def _family(n, mg, meq, B=BMAX):
    (H, f, G, bl, bu, lb, ub, xc), (A, lo, hi), refs = BO.box_reference(BMAX, n, mg, meq)
    return [v[:B] for v in (H, f, G, bl, bu, lb, ub, xc)], [v[:B] for v in (A, lo, hi)], refs[:B]


def _relx(x, xr):
    return np.abs(x - xr).max(axis=1) / np.maximum(1.0, np.abs(xr).max(axis=1))


def _rell(lam, lr):
    return np.abs(lam - lr).max(axis=1) / (1.0 + np.abs(lr).max(axis=1))


# ------------------------------------------------------------------ 1. bit for bit
@pytest.mark.parametrize("n,mg,meq", BO.SHAPES)
def test_bit_for_bit(qpb, n, mg, meq):
    for B in BATCHES:
        (H, f, G, bl, bu, lb, ub, _), _, _ = _family(n, mg, meq, B)
        got = _box(qpb, H, f, G, bl, bu, lb, ub, meq)
        assert got.lam.shape == (B, mg + n) and got.active.shape == (B, (mg + n + 31) // 32) == got.lower.shape
        _equal(got, _mat(qpb, H, f, G, bl, bu, lb, ub, meq))
        assert (got.status == OK).all()


@pytest.mark.parametrize("n,mg,meq", BO.SHAPES)
def test_bit_for_bit_shared(qpb, n, mg, meq):
    """One H and / or one G for the batch.  With one G the rows' bounds are
    redrawn around every QP's own point, so the batch stays feasible."""
    for B in BATCHES:
        (H, f, G, bl, bu, lb, ub, xc), _, _ = _family(n, mg, meq, B)
        H0, G0 = H[0], G[0]
        gx = np.einsum("ij,bj->bi", G0, xc)
        rng = np.random.default_rng([n, mg, meq, B])
        buS = gx + rng.uniform(0.05, 1.0, size=gx.shape)
        blS = gx - rng.uniform(0.05, 1.0, size=gx.shape)
        blS[:, :meq] = buS[:, :meq] = gx[:, :meq]
        ok = 0
        for Hs, Gs, lo, hi in ((H0, G, bl, bu), (H, G0, blS, buS), (H0, G0, blS, buS)):
            if mg == 0 and Gs is G0:
                Gs = None  # no rows: nothing to share
            got = _box(qpb, Hs, f, Gs, lo if Gs is not None else None, hi if Gs is not None else None, lb, ub, meq)
            _equal(got, _mat(qpb, Hs, f, Gs, lo if Gs is not None else None, hi if Gs is not None else None,
                             lb, ub, meq))
            ok += int((got.status == OK).sum())
        assert ok >= 2 * B  # the problems are solved, not rejected alike


# ------------------------------------------------------------------------ 2. parity
@pytest.mark.parametrize("n,mg,meq", BO.SHAPES)
def test_parity(qpb, n, mg, meq):
    m = mg + n
    for B in BATCHES:
        (H, f, G, bl, bu, lb, ub, _), (A, lo, hi), refs = _family(n, mg, meq, B)
        assert len(refs) == B and all(r.status == 0 for r in refs)
        x, lam, act, low, st, it = _host(_box(qpb, H, f, G, bl, bu, lb, ub, meq))
        mask, lmask = RO.unpack_bits(act, m), RO.unpack_bits(low, m)
        xr = np.array([r.x for r in refs])
        lr = np.array([r.lam for r in refs])
        ar = np.array([r.active for r in refs])
        wr = np.array([r.lower for r in refs])
        worst = {k: float(v.max()) for k, v in RO.kkt_range(H, f, A, lo, hi, meq, x, lam).items()}
        print(f"({n},{mg},{meq}) B={B}: x err {_relx(x, xr).max():.2e} lam err {_rell(lam, lr).max():.2e} "
              f"kkt {max(worst.values()):.2e} active mismatches {int((mask != ar).any(axis=1).sum())} "
              f"lower mismatches {int((lmask != wr).any(axis=1).sum())} iters {it.min()}..{it.max()}")
        assert (st == OK).all(), st
        assert np.array_equal(mask, ar)
        assert np.array_equal(lmask, wr)
        assert _relx(x, xr).max() <= X_TOL
        assert _rell(lam, lr).max() <= X_TOL
        assert all(v <= KKT_TOL for v in worst.values()), worst
        # variable j sits at mg + j: >= 0 at ub, <= 0 at lb
        assert (lam[:, mg:][(mask & ~lmask)[:, mg:]] >= 0).all() and (lam[:, mg:][lmask[:, mg:]] <= 0).all()
        assert (it <= 4 * (n + m) + 8).all()


# ------------------------------------------------------------------------ 3. bounds
@pytest.mark.parametrize("n,mg,meq", CLASSES)
def test_absent_bounds(qpb, n, mg, meq):
    B = 67
    (H, f, G, bl, bu, lb, ub, _), _, _ = _family(n, mg, meq, B)
    inf = lambda v: np.full_like(v, np.inf)  # noqa: E731
    # a None array is that side at infinity, everywhere
    _equal(_box(qpb, H, f, G, bl, bu, None, ub, meq), _box(qpb, H, f, G, bl, bu, -inf(lb), ub, meq))
    _equal(_box(qpb, H, f, G, bl, bu, lb, None, meq), _box(qpb, H, f, G, bl, bu, lb, inf(ub), meq))
    _equal(_box(qpb, H, f, G, bl, bu, None, ub, meq), _mat(qpb, H, f, G, bl, bu, None, ub, meq))
    if mg:
        _equal(_box(qpb, H, f, G, bl, bu, None, None, meq), _box(qpb, H, f, G, bl, bu, -inf(lb), inf(ub), meq))
        blx = -inf(bl)
        blx[:, :meq] = bl[:, :meq]  # an equality's bl is not read
        _equal(_box(qpb, H, f, G, None, bu, lb, ub, meq), _box(qpb, H, f, G, blx, bu, lb, ub, meq))
        _equal(_box(qpb, H, f, G, None, bu, lb, ub, meq), _mat(qpb, H, f, G, None, bu, lb, ub, meq))
        if meq == 0:
            _equal(_box(qpb, H, f, G, bl, None, lb, ub, meq), _box(qpb, H, f, G, bl, inf(bu), lb, ub, meq))
            _equal(_box(qpb, H, f, G, None, None, lb, ub, meq), _box(qpb, H, f, G, -inf(bl), inf(bu), lb, ub, meq))
    # single entries: NaN and infinities of either sign are absent sides
    rng = np.random.default_rng([n, mg, 77])
    lbn, ubn, lbi, ubi = lb.copy(), ub.copy(), lb.copy(), ub.copy()
    for arr_bad, arr_inf, fill in ((lbn, lbi, -np.inf), (ubn, ubi, np.inf)):
        hit = rng.random(arr_bad.shape) < 0.3
        kinds = rng.integers(0, 3, size=arr_bad.shape)
        arr_bad[hit] = np.choose(kinds[hit], [np.nan, np.inf, -np.inf])
        arr_inf[hit] = fill
    got = _box(qpb, H, f, G, bl, bu, lbn, ubn, meq)
    _equal(got, _box(qpb, H, f, G, bl, bu, lbi, ubi, meq))
    _equal(got, _mat(qpb, H, f, G, bl, bu, lbn, ubn, meq))
    assert (got.status == OK).all()


@pytest.mark.parametrize("n,mg,meq", CLASSES)
def test_pinned_and_crossed(qpb, n, mg, meq):
    B = 12
    (H, f, G, bl, bu, lb, ub, xc), _, _ = _family(n, mg, meq, B)
    m = mg + n
    # a pinned variable, lb_j == ub_j at the strictly feasible point: a zero-width row
    lbp, ubp = lb.copy(), ub.copy()
    j = np.arange(B) % n
    lbp[np.arange(B), j] = ubp[np.arange(B), j] = xc[np.arange(B), j]
    got = _box(qpb, H, f, G, bl, bu, lbp, ubp, meq)
    _equal(got, _mat(qpb, H, f, G, bl, bu, lbp, ubp, meq))
    x, lam, act, low, st, it = _host(got)
    # the oracle takes the pin as one more equality, e_j x = xc_j, in front of G's rows
    lbo, ubo = lbp.copy(), ubp.copy()
    lbo[np.arange(B), j], ubo[np.arange(B), j] = -np.inf, np.inf
    A, lo, hi = BO.materialise(G, bl, bu, lbo, ubo, n)
    pin = np.eye(n)[j][:, None, :]
    A = np.concatenate([pin, A], axis=1)
    pv = xc[np.arange(B), j][:, None]
    lo, hi = np.concatenate([pv, lo], axis=1), np.concatenate([pv, hi], axis=1)
    refs = [RO.range_solve(H[i], f[i], A[i], lo[i], hi[i], meq + 1, xc[i]) for i in range(B)]
    assert all(r.status == 0 for r in refs) and (st == OK).all()
    assert _relx(x, np.array([r.x for r in refs])).max() <= X_TOL
    assert np.abs(x[np.arange(B), j] - xc[np.arange(B), j]).max() <= 1e-9 * (1.0 + np.abs(xc).max())
    assert RO.unpack_bits(act, m)[np.arange(B), mg + j].all()
    # crossed beyond the threshold: INFEASIBLE from the set-up, on the QPs that have it only
    lbc = lb.copy()
    bad = np.arange(0, B, 3)
    lbc[bad, j[bad]] = ub[bad, j[bad]] + 1e-3 * (1.0 + np.abs(ub[bad, j[bad]]))
    base = _host(_box(qpb, H, f, G, bl, bu, lb, ub, meq))
    got = _box(qpb, H, f, G, bl, bu, lbc, ub, meq)
    _equal(got, _mat(qpb, H, f, G, bl, bu, lbc, ub, meq))
    x, lam, act, low, st, it = _host(got)
    assert (st[bad] == INFEASIBLE).all() and (it[bad] == 0).all()
    assert (lam[bad] == 0).all() and (act[bad] == 0).all() and (low[bad] == 0).all()
    keep = np.setdiff1d(np.arange(B), bad)
    for u, v in zip((x, lam, act, low, st, it), base):
        assert np.array_equal(u[keep].view(np.uint8), v[keep].view(np.uint8))


# ---------------------------------------------------------------------- 4. contract
@pytest.mark.parametrize("n,mg,meq", CLASSES)
def test_independence(qpb, n, mg, meq):
    B = 67
    (H, f, G, bl, bu, lb, ub, _), _, _ = _family(n, mg, meq, B)
    full = _host(_box(qpb, H, f, G, bl, bu, lb, ub, meq))
    take = lambda sol, idx: [v[idx] for v in sol]  # noqa: E731
    same = lambda a, b: all(np.array_equal(u.view(np.uint8), v.view(np.uint8)) for u, v in zip(a, b))  # noqa: E731
    # the batch size and the position in the batch
    for k in (0, 5, 66):
        s = slice(k, k + 1)
        one = _host(_box(qpb, H[s], f[s], G[s], bl[s], bu[s], lb[s], ub[s], meq))
        assert same(one, take(full, s)), k
        idx = [1, 2, 3, 4, k]
        five = _host(_box(qpb, H[idx], f[idx], G[idx], bl[idx], bu[idx], lb[idx], ub[idx], meq))
        assert same(take(five, slice(4, 5)), take(full, s)), k
    # neighbours in the same wave with NaN in H, f, G and the bounds
    Hn, fn, Gn, bln, bun, lbn, ubn = (v.copy() for v in (H, f, G, bl, bu, lb, ub))
    Hn[1] = np.nan
    fn[2] = np.nan
    lbn[6] = np.nan
    ubn[6] = np.nan
    poisoned = [1, 2, 6]
    if mg:
        Gn[5] = np.nan
        bun[9] = np.nan
        bln[9] = np.nan
        poisoned += [5, 9]
    got = _host(_box(qpb, Hn, fn, Gn, bln, bun, lbn, ubn, meq))
    keep = [k for k in range(B) if k not in poisoned]
    assert same(take(got, keep), take(full, keep))
    st = got[4]
    assert st[1] == NOT_SPD and st[2] != OK
    if mg:
        assert st[5] == NUMERICAL
    # ... as qpb_solve_range has it
    _equal(_box(qpb, Hn, fn, Gn, bln, bun, lbn, ubn, meq), _mat(qpb, Hn, fn, Gn, bln, bun, lbn, ubn, meq))


@pytest.mark.parametrize("n,mg,meq", CLASSES)
@pytest.mark.parametrize("B", (5, 67))
def test_every_element_written_and_nothing_beyond(qpb, n, mg, meq, B):
    (H, f, G, bl, bu, lb, ub, _), _, _ = _family(n, mg, meq, B)
    m = mg + n
    w = (m + 31) // 32
    PAD = 64  # guard elements on both sides of every output
    dev = torch.device("cuda")
    shapes = ((B, n), (B, m), (B, w), (B, w), (B,), (B,))
    dtypes = (torch.float64, torch.float64, torch.int32, torch.int32, torch.int32, torch.int32)
    bufs, views = [], []
    for shp, dt in zip(shapes, dtypes):
        count = int(np.prod(shp))
        buf = torch.empty(count + 2 * PAD, dtype=dt, device=dev)
        buf.view(torch.uint8).fill_(0xA5)
        bufs.append(buf)
        views.append(buf[PAD:PAD + count].view(shp))
    out = qpb.RangeSolution(*views)
    # a failing QP in the batch: its outputs are written as well
    Hb = H.copy()
    Hb[B - 1] = np.nan
    got = _box(qpb, Hb, f, G, bl, bu, lb, ub, meq, out=out)
    torch.cuda.synchronize()
    assert all(g.data_ptr() == v.data_ptr() for g, v in zip(got, views))
    for name, buf, view in zip(NAMES, bufs, views):
        raw = buf.view(torch.uint8).cpu().numpy()
        isz = buf.element_size()
        assert (raw[:PAD * isz] == 0xA5).all() and (raw[-PAD * isz:] == 0xA5).all(), (name, "written outside")
        inner = raw[PAD * isz:-PAD * isz].reshape(-1, isz)
        assert not (inner == 0xA5).all(axis=1).any(), (name, "elements never written")
    assert got.status[B - 1].item() == NOT_SPD and (got.status[:B - 1] == OK).all()
    _equal(got, _mat(qpb, Hb, f, G, bl, bu, lb, ub, meq))


@pytest.mark.parametrize("n,mg,meq", CLASSES)
def test_failure_statuses(qpb, n, mg, meq):
    B = 8
    (H, f, G, bl, bu, lb, ub, _), _, _ = _family(n, mg, meq, B)
    Hn, Gn = H.copy(), G.copy()
    Hn[3, 0, 0] = np.nan
    if mg:
        Gn[4, mg - 1, n - 1] = np.nan
    got = _box(qpb, Hn, f, Gn, bl, bu, lb, ub, meq)
    _equal(got, _mat(qpb, Hn, f, Gn, bl, bu, lb, ub, meq))
    st = _host(got)[4]
    assert st[3] == NOT_SPD
    if mg:
        assert st[4] == NUMERICAL
    assert (np.delete(st, [3, 4] if mg else [3]) == OK).all()
    # max_iter = 1: the cap's contract, and the default cap is the materialised problem's
    got = _box(qpb, H, f, G, bl, bu, lb, ub, meq, max_iter=1)
    _equal(got, _mat(qpb, H, f, G, bl, bu, lb, ub, meq, max_iter=1))
    assert (got.status == MAX_ITER).all() and (got.iters == 1).all()


# ------------------------------------------------------------------------ 5. limits
@pytest.mark.parametrize("n,mg", [(33, 0), (32, 33)])
def test_limits(qpb, n, mg):
    B = 2
    H = np.broadcast_to(np.eye(n), (B, n, n)).copy()
    f = np.ones((B, n))
    G = np.ones((B, mg, n)) if mg else None
    b = np.ones((B, mg)) if mg else None
    with pytest.raises(qpb.QPBError) as e:
        qpb.solve_range_box(*_dev(H, f, G, None if b is None else -b, b, -np.ones((B, n)), np.ones((B, n))))
    assert e.value.code == qpb.ERR_UNSUPPORTED
    # one size below, the call runs
    n2, mg2 = (32, 0) if mg == 0 else (32, 32)
    H = np.broadcast_to(np.eye(n2), (B, n2, n2)).copy()
    G = np.ones((B, mg2, n2)) if mg2 else None
    b = 100.0 * np.ones((B, mg2)) if mg2 else None
    sol = qpb.solve_range_box(*_dev(H, np.ones((B, n2)), G, None if b is None else -b, b, -np.ones((B, n2)) / 2,
                                    np.ones((B, n2))))
    torch.cuda.synchronize()
    assert (sol.status == OK).all() and (sol.x + 0.5).abs().max().item() <= 1e-12
