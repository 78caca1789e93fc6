"""The other half of qpb.h's contract, on every kernel route: failure statuses,
the max_iter / feas_tol / iters == NULL limits, inputs with b < 0, non-finite
inputs, isolation between the QPs of one launch, and the output footprint.

Routes = the smallest shapes that reach each kernel form (DENSE below; BOX_N
for qpb_solve_box).  Bars are the project's own: x and lambda within 1e-6
relative of the KKT-certified oracle (oracle/oracle.py), active sets bit-exact,
KKT residuals of the GPU's answer <= 1e-9.  "Bitwise" comparisons are between
two launches of the same kernel on the same QP.

Every input is a legal call under qpb.h and every loop is bounded by max_iter.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

X_TOL = 1e-6
KKT_TOL = 1e-9
OK, MAX_ITER, NOT_SPD, INFEASIBLE, NUMERICAL = 0, 1, 2, 3, 4
FLAG_MIXED, FLAG_DIAG_WAVE = 32, 256

# (kernel form, n, m, batch, qpb_desc.flags)
DENSE = [
    ("gi_dense-mr1-padded", 7, 14, 37, 0),
    ("gi_dense-mr2-padded", 13, 26, 37, 0),
    ("gi_dense-n16-mr1", 16, 16, 37, 0),
    ("gi_dense-full", 16, 32, 37, 0),
    ("gi_wave-diag", 7, 14, 13, FLAG_DIAG_WAVE),
    ("gi_wave-20x33", 20, 33, 13, 0),
    ("gi_wave-32x64", 32, 64, 13, 0),
    ("gi_mixed", 20, 33, 13, FLAG_MIXED),
    ("gi_gram-33x40", 33, 40, 6, 0),
    ("gi_gram-48x96", 48, 96, 6, 0),
]
BOX_N = [7, 16, 20, 40]  # gi_box padded and full, gi_wave's BOX form, gi_gram's
BOX_B = 13
dense_routes = pytest.mark.parametrize("route", DENSE, ids=[r[0] for r in DENSE])
box_routes = pytest.mark.parametrize("n", BOX_N)


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    return q


def _cap(n, m):
    return 4 * (n + m) + 8  # qpb_desc.max_iter's default


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda() for a in arrays]


def _host(sol):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in sol]


def _solve(qpb, H, f, A, b, flags=0, **kw):
    return _host(qpb.solve(*_dev(H, f, A, b), flags=flags, **kw))


def _solve_box(qpb, H, f, lb, ub, **kw):
    return _host(qpb.solve_box(*_dev(H, f, lb, ub), **kw))


def _box_dense(lb, ub):
    B, n = lb.shape
    A = np.concatenate([np.broadcast_to(np.eye(n), (B, n, n)), np.broadcast_to(-np.eye(n), (B, n, n))], axis=1).copy()
    return A, np.concatenate([ub, -lb], axis=1)


def _same(a, b):
    """Bitwise equality of two solutions (NaN payloads included)."""
    return all(np.array_equal(u.view(np.uint8), v.view(np.uint8)) for u, v in zip(a, b))


_ORACLE = {}


def _oracle(key, H, f, A, b, x0):
    """The oracle's answers for one batch, computed once per session and shared
    (never modified) by the tests that need them."""
    import oracle as O
    if key not in _ORACLE:
        refs = [O.active_set_solve(H[i], f[i], A[i], b[i], x0=x0[i]) for i in range(len(f))]
        assert all(r.status == 0 for r in refs), key
        _ORACLE[key] = refs
    return _ORACLE[key]


def _kkt(H, f, A, b, x, lam):
    import oracle as O
    return {k: float(v.max()) for k, v in O.kkt_residuals(H, f, A, b, x, lam).items()}


def _check_parity(qpb, H, f, A, b, sol, refs, what=""):
    """status OK, x and lambda within X_TOL of the oracle, active set bit-exact,
    KKT residuals of the GPU's own answer <= KKT_TOL."""
    x, lam, act, st, it = sol
    m = A.shape[1]
    assert (st == OK).all(), (what, st)
    mask = qpb.active_mask_to_bool(act, m)
    xr = np.array([r.x for r in refs])
    lr = np.array([r.lam for r in refs])
    ar = np.array([r.active for r in refs])
    ex = np.abs(x - xr).max(axis=1) / np.maximum(1.0, np.abs(xr).max(axis=1))
    el = np.abs(lam - lr).max(axis=1) / (1.0 + np.abs(lr).max(axis=1))
    worst = _kkt(H, f, A, b, x, lam)
    print(f"{what}: x err {ex.max():.2e} lam err {el.max():.2e} kkt {max(worst.values()):.2e} "
          f"mask mismatches {int((mask != ar).any(axis=1).sum())} iters {it.min()}..{it.max()}")
    assert ex.max() <= X_TOL, (what, ex)
    assert el.max() <= X_TOL, (what, el)
    assert np.array_equal(mask, ar), (what, np.nonzero((mask != ar).any(axis=1)))
    assert all(v <= KKT_TOL for v in worst.values()), (what, worst)
    assert (it <= _cap(H.shape[1], m)).all()


def _check_setup_failure(qpb, sol, idx, m, what):
    """QPs that fail in the set-up (NOT_SPD, a zero row with b < 0, a NaN row
    of A): no iteration ran, lam = 0, the active set is empty (qpb.h)."""
    x, lam, act, st, it = sol
    mask = qpb.active_mask_to_bool(act, m)
    assert (it[idx] == 0).all(), (what, it[idx])
    assert (lam[idx] == 0).all(), (what, lam[idx])
    assert not mask[idx].any(), (what, mask[idx])


def _check_dual_iterate(qpb, H, f, A, b, sol, idx, what):
    """QPs that stop inside the iteration without a solution (MAX_ITER,
    discovered INFEASIBLE) hold the dual iterate reached (qpb.h): x and lam
    finite, lam >= 0 and zero outside the active mask, and stationarity
    |H x + f + A^T lam| <= KKT_TOL relative -- every kernel recovers
    x = -H^{-1} (f + A^T lam) from the multipliers it writes."""
    x, lam, act, st, it = sol
    mask = qpb.active_mask_to_bool(act, A.shape[1])
    assert np.isfinite(x[idx]).all() and np.isfinite(lam[idx]).all(), what
    stat = _kkt(H[idx], f[idx], A[idx], b[idx], x[idx], lam[idx])["stat"]
    print(f"{what}: min lam {lam[idx].min():.3e}, active {mask[idx].sum(axis=1).tolist()}, stationarity {stat:.2e}")
    assert (lam[idx] >= 0).all(), (what, lam[idx].min())
    assert (lam[idx][~mask[idx]] == 0).all(), what
    assert stat <= KKT_TOL, (what, stat)


# ------------------------------------------------------------- a. negative b
@dense_routes
def test_negative_b(qpb, route):
    """family_shifted: the feasible region does not contain x = 0 and about
    30 % of b is negative, so the violation threshold -tol (|a| + |b|) and the
    slack set-up s = b + D y see b < 0.  Full parity with the oracle started
    from the family's feasible point."""
    import oracle as O
    name, n, m, B, flags = route
    H, f, A, b, xc = O.family_shifted(1000 + n + m, B, n, m)
    assert (b < 0).mean() >= 0.2
    refs = _oracle(("shifted", n, m, B), H, f, A, b, xc)
    _check_parity(qpb, H, f, A, b, _solve(qpb, H, f, A, b, flags), refs, name)


def _shifted_box(n, B, seed):
    """family_conditioned's H and f with lb = c - w1, ub = c + w2,
    c ~ U(-20, 20), w ~ U(0.5, 1.5) * 10: the box need not contain 0."""
    import oracle as O
    H, f, _, _ = O.family_conditioned(seed, B, n, box=10.0)
    rs = np.random.default_rng([seed, 77])
    c = rs.uniform(-20.0, 20.0, (B, n))
    lb = c - rs.uniform(0.5, 1.5, (B, n)) * 10.0
    ub = c + rs.uniform(0.5, 1.5, (B, n)) * 10.0
    return H, f, lb, ub, c


@box_routes
def test_negative_b_box(qpb, n):
    """qpb_solve_box on boxes that need not contain 0 (bounds of either sign):
    parity with the oracle on the dense form A = [I; -I], b = [ub; -lb], and
    with qpb_solve on that form."""
    H, f, lb, ub, c = _shifted_box(n, BOX_B, 1100 + n)
    A, b = _box_dense(lb, ub)
    assert (b < 0).mean() >= 0.2
    refs = _oracle(("shifted_box", n, BOX_B), H, f, A, b, c)
    box = _solve_box(qpb, H, f, lb, ub)
    _check_parity(qpb, H, f, A, b, box, refs, f"box n={n}")
    dense = _solve(qpb, H, f, A, b)
    _check_parity(qpb, H, f, A, b, dense, refs, f"dense form n={n}")
    assert np.array_equal(box[2], dense[2])
    assert (np.abs(box[0] - dense[0]).max(axis=1) <= X_TOL * np.maximum(1.0, np.abs(dense[0]).max(axis=1))).all()
    assert (np.abs(box[1] - dense[1]).max(axis=1) <= X_TOL * (1.0 + np.abs(dense[1]).max(axis=1))).all()


# ------------------------------------------------ b. discovered infeasibility
def _farkas_k(route, kk):
    name, n, m, B, flags = route
    return min({"1": 1, "2": 2, "n": n, "n+1": n + 1}[kk], m - 1)


# k in {1, 2, n, min(n + 1, m - 1)}, clamped to m - 1; a clamped k that repeats the one before it is left out
FARKAS = [(r, kk) for r in DENSE for kk, prev in (("1", None), ("2", "1"), ("n", "2"), ("n+1", "n"))
          if prev is None or _farkas_k(r, kk) != _farkas_k(r, prev)]


@pytest.mark.parametrize("route,kk", FARKAS, ids=[f"{r[0]}-{kk}" for r, kk in FARKAS])
def test_discovered_infeasibility(qpb, route, kk):
    """family_farkas: row m-1 = -sum_{i<k} y_i a_i, so no single row shows the
    infeasibility: the iteration has to find it (the t1 = t2 = inf exit).
    b_inf: every QP INFEASIBLE within the default cap, holding the dual
    iterate it had reached (_check_dual_iterate).  b_feas (the same
    linearly dependent rows, one entry of b changed): every QP OK with full
    oracle parity -- a kernel cannot pass by rejecting every dependent row.
    k is clamped to m - 1 (row m - 1 is the dependent one)."""
    import oracle as O
    name, n, m, B, flags = route
    k = _farkas_k(route, kk)
    H, f, A, b_inf, b_feas, xc, cert = O.family_farkas(1200 + n + m, B, n, m, k)
    x, lam, act, st, it = sol = _solve(qpb, H, f, A, b_inf, flags)
    print(f"{name} k={k}: b_inf statuses {np.bincount(st, minlength=5).tolist()} iters {it.min()}..{it.max()}")
    assert (st == INFEASIBLE).all(), st
    assert (it <= _cap(n, m)).all() and (it >= 1).all()
    _check_dual_iterate(qpb, H, f, A, b_inf, sol, np.arange(B), f"{name} k={k} b_inf")
    refs = _oracle(("farkas", n, m, B, k), H, f, A, b_feas, xc)
    _check_parity(qpb, H, f, A, b_feas, _solve(qpb, H, f, A, b_feas, flags), refs, f"{name} k={k} twin")


# ------------------------------------------------------------------ c. max_iter
def _vertex_family(n, m, B, seed, scale=100.0):
    """tests/test_gpu_active_set.py's vertex family (H = I + 0.1 B^T B / n,
    f ~ scale N(0, I), unit-norm random rows, b ~ U[0.1, 1)) with f scaled per
    QP by 10^U(-2, 0), and by 1e-5 for every fifth QP: from QPs whose
    unconstrained minimiser is feasible (one iteration) to full active sets
    reached through drops, so the iteration counts spread over the batch."""
    rs = np.random.default_rng(seed)
    Bm = rs.standard_normal((B, n, n))
    H = np.eye(n) + 0.1 * np.einsum("bki,bkj->bij", Bm, Bm) / n
    f = scale * rs.standard_normal((B, n))
    A = rs.standard_normal((B, m, n))
    A /= np.linalg.norm(A, axis=2, keepdims=True)
    b = rs.uniform(0.1, 1.0, (B, m))
    g = 10.0 ** rs.uniform(-2.0, 0.0, B)
    g[4::5] = 1e-5
    return H, f * g[:, None], A, b


def _check_capped(qpb, name, Hh, fh, Ah, bh, m, full, solve):
    """full: the uncapped solution; solve(max_iter) the same launch with a cap."""
    it_full = full[4]
    assert (full[3] == OK).all(), full[3]
    K = int(np.median(it_full))
    B = len(it_full)
    done, cut = it_full <= K, it_full > K
    print(f"{name}: uncapped iters {sorted(it_full.tolist())} K={K}")
    assert 4 * done.sum() >= B and 4 * cut.sum() >= B, (it_full, K)
    x, lam, act, st, it = capped = solve(K)
    assert (st[done] == OK).all() and (st[cut] == MAX_ITER).all(), (st, it_full, K)
    for u, v in zip(capped, full):
        assert np.array_equal(u[done].view(np.uint8), v[done].view(np.uint8))
    assert (it[cut] == K).all(), it
    _check_dual_iterate(qpb, Hh, fh, Ah, bh, capped, cut, f"{name} at MAX_ITER")
    one = solve(1)
    assert (it_full == 1).any()
    assert np.array_equal(one[3] == OK, it_full == 1), (one[3], it_full)
    assert (one[3][it_full > 1] == MAX_ITER).all() and (one[4] == 1).all()


@dense_routes
def test_max_iter(qpb, route):
    """max_iter = K = median of the uncapped iteration counts: the QPs that
    need <= K iterations are OK and bitwise unchanged in all five outputs, the
    others end MAX_ITER with iters == K, finite x and lambda, lambda >= 0 and
    zero outside the active mask; each class holds at least a quarter of the
    batch.  max_iter = 1: OK exactly for the QPs that need one iteration.

    Stationarity at MAX_ITER (|H x + f + A^T lam| <= 1e-9 relative) is
    asserted on every route: gi_dense, gi_wave, gi_gram and the three box
    kernels all recover x = -H^{-1} (f + A^T lam) from the multipliers they
    write, and gi_mixed's MAX_ITER answers come from gi_wave's re-solve."""
    name, n, m, B, flags = route
    H, f, A, b = _vertex_family(n, m, B, 1300 + n + m)
    full = _solve(qpb, H, f, A, b, flags)
    _check_capped(qpb, name, H, f, A, b, m, full, lambda K: _solve(qpb, H, f, A, b, flags, max_iter=K))


@box_routes
def test_max_iter_box(qpb, n):
    """test_max_iter on qpb_solve_box (unit box, the vertex family's H and f)."""
    H, f, _, _ = _vertex_family(n, 1, BOX_B, 1400 + n)
    lb, ub = -np.ones((BOX_B, n)), np.ones((BOX_B, n))
    A, b = _box_dense(lb, ub)
    full = _solve_box(qpb, H, f, lb, ub)
    _check_capped(qpb, f"box n={n}", H, f, A, b, 2 * n, full, lambda K: _solve_box(qpb, H, f, lb, ub, max_iter=K))


# ------------------------------------------------------------------ d. feas_tol
@dense_routes
def test_feas_tol(qpb, route):
    """H = I, row 0 = e_0 with b_0 placed so that the unconstrained minimiser
    -f violates it by 1e-7 (1 + |b_0|) (the other rows are far away).  Default
    tolerance 1e-10: row 0 is active and x_0 = b_0.  feas_tol = 1e-6: nothing
    is violated, the mask is empty and x = -f."""
    name, n, m, B, flags = route
    rs = np.random.default_rng(1500 + n + m)
    H = np.broadcast_to(np.eye(n), (B, n, n)).copy()
    A = rs.standard_normal((B, m, n))
    A /= np.linalg.norm(A, axis=2, keepdims=True)
    A[:, 0] = 0.0
    A[:, 0, 0] = 1.0
    b = np.full((B, m), 1e3)
    b[:, 0] = rs.uniform(-3.0, 3.0, B)
    f = rs.uniform(-1.0, 1.0, (B, n))
    f[:, 0] = -(b[:, 0] + 1e-7 * (1.0 + np.abs(b[:, 0])))
    x, lam, act, st, it = _solve(qpb, H, f, A, b, flags)
    mask = qpb.active_mask_to_bool(act, m)
    assert (st == OK).all(), st
    assert mask[:, 0].all() and (mask.sum(axis=1) == 1).all()
    assert np.abs(x[:, 0] - b[:, 0]).max() <= 1e-12 and np.abs(x[:, 1:] + f[:, 1:]).max() <= 1e-12
    assert np.allclose(lam[:, 0], -f[:, 0] - b[:, 0], rtol=1e-6, atol=0)
    x, lam, act, st, it = _solve(qpb, H, f, A, b, flags, feas_tol=1e-6)
    assert (st == OK).all(), st
    assert not qpb.active_mask_to_bool(act, m).any() and (lam == 0).all()
    assert np.abs(x + f).max() <= 1e-12


# -------------------------------------------------------------- e. iters = NULL
@dense_routes
def test_iters_null(qpb, route):
    """qpb_solve with iters == NULL writes the same x, lam, active and status
    as a call that passes iters."""
    import oracle as O
    name, n, m, B, flags = route
    H, f, A, b, _ = O.family_shifted(1000 + n + m, B, n, m)
    want = _solve(qpb, H, f, A, b, flags)
    ins = _dev(H, f, A, b)
    x = torch.zeros((B, n), dtype=torch.float64, device="cuda")
    lam = torch.zeros((B, m), dtype=torch.float64, device="cuda")
    act = torch.zeros((B, (m + 31) // 32), dtype=torch.int32, device="cuda")
    st = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    d = qpb.Desc(n, m, B, 0, flags, 0.0)
    rc = qpb.solve_raw(d, [t.data_ptr() for t in ins + [x, lam, act, st]] + [0],
                       torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    got = _host([x, lam, act, st])
    assert _same(got, want[:4])


# ------------------------------------------------------------- f. m = 0, gi_gram
def test_unconstrained_gram(qpb):
    """m = 0 at n = 40 (gi_gram): x = -H^{-1} f within 1e-9 relative."""
    import oracle as O
    H, f, _, _ = O.family_conditioned(1600, 6, 40, box=10.0)
    sol = qpb.solve(*_dev(H, f))
    x, lam, act, st, it = _host(sol)
    ref = np.linalg.solve(H, -f[:, :, None])[:, :, 0]
    assert (st == OK).all(), st
    assert (np.abs(x - ref).max(axis=1) <= 1e-9 * np.abs(ref).max(axis=1)).all()
    assert lam.shape == (6, 0) and act.shape == (6, 0)


# ----------------------------------------------------------------- g. isolation
KINDS = ["ok", "zero_iter", "vertex", "farkas", "neg_H", "zero_row", "nan_H"]
KIND_STATUS = {"ok": OK, "zero_iter": OK, "vertex": OK, "farkas": INFEASIBLE, "neg_H": NOT_SPD,
               "zero_row": INFEASIBLE, "nan_H": NOT_SPD}


def _mixed_batch(n, m, B, seed):
    """QP i is of kind KINDS[i % 7], so every wavefront of the four-QP kernel
    mixes finished, long-running, failed and NaN QPs."""
    import oracle as O
    H, f, A, b, _ = O.family_shifted(seed, B, n, m)
    Hv, fv, Av, bv = _vertex_family(n, m, B, seed + 1)
    k2 = min(2, m - 1)
    Hf, ff, Af, bf, _, _, _ = O.family_farkas(seed + 2, B, n, m, k2)
    kinds = [KINDS[i % len(KINDS)] for i in range(B)]
    for i, kind in enumerate(kinds):
        if kind == "zero_iter":
            b[i] = 1e6
        elif kind == "vertex":
            H[i], f[i], A[i], b[i] = Hv[i], 100.0 * fv[i] / np.abs(fv[i]).max(), Av[i], bv[i]
        elif kind == "farkas":
            H[i], f[i], A[i], b[i] = Hf[i], ff[i], Af[i], bf[i]
        elif kind == "neg_H":
            H[i] = -H[i]
        elif kind == "zero_row":
            A[i, m // 2] = 0.0
            b[i, m // 2] = -1.0
        elif kind == "nan_H":
            H[i, 0, n - 1] = H[i, n - 1, 0] = np.nan
    return H, f, A, b, kinds


ISO_MIN_BATCH = 13  # at least one QP of each of the seven kinds (gi_gram's routes: 13, not 6)


@dense_routes
def test_isolation(qpb, route):
    """One launch mixing the seven kinds: every QP ends with the status its
    kind dictates, and the outputs of the OK kinds are bitwise those of a
    launch that holds the OK QPs alone, in reverse order (other partners in
    the wavefront, other slots, another position in gi_gram's queue).  The
    failed QPs hold what qpb.h states: the set-up failures (-H, zero row, NaN
    in H) no iteration, lam = 0 and an empty active set, the Farkas QPs the
    dual iterate they reached.  The batch is 13 on gi_gram's routes so that
    all seven kinds occur."""
    name, n, m, B, flags = route
    B = max(B, ISO_MIN_BATCH)
    H, f, A, b, kinds = _mixed_batch(n, m, B, 1700 + n + m)
    sol = _solve(qpb, H, f, A, b, flags)
    st, it = sol[3], sol[4]
    print(f"{name}: " + " ".join(f"{k}:{s}/{i}" for k, s, i in zip(kinds, st, it)))
    assert st.tolist() == [KIND_STATUS[k] for k in kinds], list(zip(kinds, st))
    vert = [i for i, k in enumerate(kinds) if k == "vertex"]
    assert (it[vert] > 4).all(), it[vert]  # still iterating when its partners are long done
    assert (it[[i for i, k in enumerate(kinds) if k == "zero_iter"]] == 1).all()
    good = np.array([i for i, k in enumerate(kinds) if KIND_STATUS[k] == OK])[::-1].copy()
    alone = _solve(qpb, H[good], f[good], A[good], b[good], flags)
    assert _same([v[good] for v in sol], alone)
    res = _kkt(H[good], f[good], A[good], b[good], sol[0][good], sol[1][good])
    assert all(v <= KKT_TOL for v in res.values()), res
    early = np.array([i for i, k in enumerate(kinds) if k in ("neg_H", "zero_row", "nan_H")])
    _check_setup_failure(qpb, sol, early, m, name)
    fark = np.array([i for i, k in enumerate(kinds) if k == "farkas"])
    assert (it[fark] >= 1).all()
    _check_dual_iterate(qpb, H, f, A, b, sol, fark, f"{name} farkas kind")


# --------------------------------------------------------- h. non-finite inputs
POISONS = ["H_nan", "H_pinf", "H_ninf", "f_nan", "f_pinf", "f_ninf", "A_nan"]


def _poison(H, f, A, j, kind, n, m):
    nan, inf = np.nan, np.inf
    if kind == "H_nan":
        H[j, 1 % n, 1 % n] = nan
    elif kind == "H_pinf":
        H[j, 0, 0] = inf
    elif kind == "H_ninf":
        H[j, 0, n - 1] = H[j, n - 1, 0] = -inf
    elif kind == "f_nan":
        f[j, n - 1] = nan
    elif kind == "f_pinf":
        f[j, 0] = inf
    elif kind == "f_ninf":
        f[j, n // 2] = -inf
    elif kind == "A_nan":
        A[j, m - 1, n // 2] = nan


@dense_routes
def test_non_finite_inputs(qpb, route):
    """A NaN or +-Inf in H or f, or a NaN in a row of A, ends that QP with a
    status other than OK and leaves every other QP of the launch bitwise
    unchanged.  A NaN row of A is QPB_NUMERICAL from the set-up; that QP and
    every QPB_NOT_SPD one ran no iteration and has lam = 0 and an empty
    active set.  A
    NaN in b means the row is absent: all outputs equal those of the same
    launch with that b = +inf."""
    import oracle as O
    name, n, m, B, flags = route
    H, f, A, b, _ = O.family_shifted(1000 + n + m, B, n, m)
    clean = _solve(qpb, H, f, A, b, flags)
    assert (clean[3] == OK).all()
    seen = {}
    for t, kind in enumerate(POISONS):
        j = (2 * t + 1) % B
        Hp, fp, Ap = H.copy(), f.copy(), A.copy()
        _poison(Hp, fp, Ap, j, kind, n, m)
        sol = _solve(qpb, Hp, fp, Ap, b, flags)
        seen[kind] = int(sol[3][j])
        if kind == "A_nan" or seen[kind] == NOT_SPD:  # failed in the set-up
            _check_setup_failure(qpb, sol, np.array([j]), m, f"{name} {kind}")
        others = np.arange(B) != j
        assert _same([v[others] for v in sol], [v[others] for v in clean]), kind
    print(f"{name}: " + " ".join(f"{k}:{s}" for k, s in seen.items()))
    assert all(s != OK for s in seen.values()), seen
    assert seen["A_nan"] == NUMERICAL, seen
    # NaN in b: the row is absent.  A row that is active in the clean answer,
    # so that its absence changes the answer.
    mask = qpb.active_mask_to_bool(clean[2], m)
    j = int(np.argmax(mask.sum(axis=1)))
    assert mask[j].any()
    r = int(np.argmax(mask[j]))
    bn, bi = b.copy(), b.copy()
    bn[j, r], bi[j, r] = np.nan, np.inf
    got, want = _solve(qpb, H, f, A, bn, flags), _solve(qpb, H, f, A, bi, flags)
    assert (want[3] == OK).all() and not qpb.active_mask_to_bool(want[2], m)[j, r]
    assert not np.array_equal(want[0][j], clean[0][j])
    assert _same(got, want)


@box_routes
def test_non_finite_inputs_box(qpb, n):
    """qpb_solve_box: a NaN or +-Inf in H or f ends that QP with a status
    other than OK and leaves the others bitwise unchanged."""
    H, f, lb, ub, _ = _shifted_box(n, BOX_B, 1100 + n)
    clean = _solve_box(qpb, H, f, lb, ub)
    seen = {}
    for t, kind in enumerate(POISONS[:6]):
        j = (2 * t + 1) % BOX_B
        Hp, fp = H.copy(), f.copy()
        _poison(Hp, fp, None, j, kind, n, 2 * n)
        sol = _solve_box(qpb, Hp, fp, lb, ub)
        seen[kind] = int(sol[3][j])
        if seen[kind] == NOT_SPD:
            _check_setup_failure(qpb, sol, np.array([j]), 2 * n, f"box n={n} {kind}")
        others = np.arange(BOX_B) != j
        assert _same([v[others] for v in sol], [v[others] for v in clean]), kind
    print(f"box n={n}: " + " ".join(f"{k}:{s}" for k, s in seen.items()))
    assert all(s != OK for s in seen.values()), seen


# ------------------------------------------------------------ i. output footprint
GUARD = 256
FILL = 0xA5


class _Guarded:
    """The five outputs as views into larger byte buffers filled with 0xA5,
    each with GUARD bytes of the same fill on both sides."""

    def __init__(self, B, n, m):
        self.bufs = []

        def view(shape, dtype):
            nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
            buf = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
            self.bufs.append((buf, nbytes))
            return buf[GUARD:GUARD + nbytes].view(dtype).view(shape)

        self.out = (view((B, n), torch.float64), view((B, m), torch.float64),
                    view((B, (m + 31) // 32), torch.int32), view((B,), torch.int32), view((B,), torch.int32))

    def check(self, what):
        torch.cuda.synchronize()
        for name, (buf, nbytes) in zip(("x", "lam", "active", "status", "iters"), self.bufs):
            raw = buf.cpu().numpy()
            assert (raw[:GUARD] == FILL).all() and (raw[GUARD + nbytes:] == FILL).all(), (what, name, "guard written")
            word = 8 if name in ("x", "lam") else 4
            left = (raw[GUARD:GUARD + nbytes].reshape(-1, word) == FILL).all(axis=1)
            assert not left.any(), (what, name, "elements never written", np.nonzero(left)[0])


@dense_routes
def test_output_footprint(qpb, route):
    """test_isolation's mixed batch (ragged: 37 or 13 QPs) written into views
    with guard bands: the kernel writes nothing outside the five outputs and
    leaves no element of any of them unwritten, whatever the QP's status."""
    name, n, m, B, flags = route
    B = max(B, ISO_MIN_BATCH)
    H, f, A, b, kinds = _mixed_batch(n, m, B, 1700 + n + m)
    g = _Guarded(B, n, m)
    out = qpb.Solution(*g.out)
    qpb.solve(*_dev(H, f, A, b), flags=flags, out=out)
    g.check(name)
    st = out.status.cpu().numpy()
    assert st.tolist() == [KIND_STATUS[k] for k in kinds]
    # and a capped launch: MAX_ITER QPs are written in full too
    g = _Guarded(B, n, m)
    out = qpb.Solution(*g.out)
    qpb.solve(*_dev(H, f, A, b), flags=flags, out=out, max_iter=2)
    g.check(name + " capped")
    assert (out.status.cpu().numpy() == MAX_ITER).any()


@box_routes
def test_output_footprint_box(qpb, n):
    """qpb_solve_box with OK, NOT_SPD, NaN and empty-box (lb > ub) QPs in one
    ragged launch: guards untouched, every output element written."""
    H, f, lb, ub, _ = _shifted_box(n, BOX_B, 1100 + n)
    H[1::4] *= -1.0
    H[2::4, 0, 0] = np.nan
    lb[3::4, n - 1] = ub[3::4, n - 1] + 1.0
    g = _Guarded(BOX_B, n, 2 * n)
    out = qpb.Solution(*g.out)
    qpb.solve_box(*_dev(H, f, lb, ub), out=out)
    g.check(f"box n={n}")
    st = out.status.cpu().numpy()
    print(f"box n={n}: statuses {st.tolist()}")
    assert (st[0::4] == OK).all() and (st[1::4] == NOT_SPD).all() and (st[2::4] != OK).all()
    assert (st[3::4] == INFEASIBLE).all()
    # the failed QPs hold what qpb.h states
    sol = _host(out)
    idx = np.arange(BOX_B)
    _check_setup_failure(qpb, sol, idx[st == NOT_SPD], 2 * n, f"box n={n}")
    A, b = _box_dense(lb, ub)
    assert (sol[4][3::4] >= 1).all()
    _check_dual_iterate(qpb, H, f, A, b, sol, idx[3::4], f"box n={n} empty box")


# ------------------------------------------------------------ status precedence
@dense_routes
def test_status_precedence(qpb, route):
    """qpb.h: QPB_NOT_SPD takes precedence over QPB_NUMERICAL (a NaN row of A),
    that over QPB_INFEASIBLE (a zero row with b < 0); all three are set-up
    failures."""
    import oracle as O
    name, n, m, B, flags = route
    H, f, A, b, _ = O.family_shifted(1000 + n + m, 5, n, m)
    for i in (1, 2, 3):  # QP 0 and 4 stay clean
        A[i, 0] = 0.0
        b[i, 0] = -1.0  # zero row, b < 0
    A[1, m - 1, 0] = A[2, m - 1, 0] = np.nan
    H[1] = -H[1]
    sol = _solve(qpb, H, f, A, b, flags)
    assert sol[3].tolist() == [OK, NOT_SPD, NUMERICAL, INFEASIBLE, OK], sol[3]
    _check_setup_failure(qpb, sol, np.array([1, 2, 3]), m, name)
