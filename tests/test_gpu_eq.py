"""qpb_solve_eq on the GPU: rows 0 .. meq-1 of A are equalities, in the EQ
forms of the two wavefront-level kernels (gi_dense: n <= 16, m <= 32, four QPs
per wavefront; gi_wave: n <= 32, m <= 64).

The reference is tests/eq_oracle.py (a null-space reduction onto the unchanged
oracle.active_set_solve) and its mixed KKT certificate.  Bars are the
project's: x and lambda within 1e-6 relative, inequality active sets
bit-exact, certificate <= 1e-9.  "Bitwise" compares two launches on the same
QP.  Shapes are the smallest that reach each code path; the batch of 67 leaves
the four-per-wave kernel a ragged last wave.

iters counts loop trips: one per row taken or left out, one per partial step
(a DROP), and the last one that finds nothing violated.  So a solve without a
DROP ends with iters = set bits + 1, and `iters > set bits + 1` is what shows a
DROP (the plain `iters > set bits` holds for every QP).  The parity test asserts
both.  The stricter one cannot hold at n - meq = 1, whatever the seed: with one
free dimension the feasible set is an interval, every violated row is a bound
on the same line, and the kernels' steepest-edge key -s / |D[p, q:]| is the
distance to that bound, so the first row taken is the binding one and nothing
is ever dropped ((16, 32, 15): 0 of 67 QPs on the MI355X).  It is asserted for
n - meq >= 2, where 1 to 28 of the 67 QPs took a DROP.
"""
import ctypes

import numpy as np
import pytest

import eq_oracle as EO

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

X_TOL = 1e-6
KKT_TOL = 1e-9
OK, MAX_ITER, NOT_SPD, INFEASIBLE, NUMERICAL = 0, 1, 2, 3, 4
B = 67

# (n, m, meq)
DENSE_SHAPES = [(16, 32, 4), (16, 32, 1), (16, 32, 15), (16, 32, 16), (16, 16, 3), (7, 13, 3), (1, 2, 1)]
WAVE_SHAPES = [(16, 33, 5), (20, 33, 5), (32, 64, 8), (32, 64, 32)]
# seed of a parity shape: 11 + n + meq (none needed another to show a DROP)
SEED = {s: 11 + s[0] + s[2] for s in DENSE_SHAPES + WAVE_SHAPES}


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    return q


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda() for a in arrays]


def _host(sol):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in sol]


FILL8 = np.frombuffer(bytes([0xA5] * 8), dtype=np.int64)[0]
FILL4 = np.frombuffer(bytes([0xA5] * 4), dtype=np.int32)[0]


def _filled(qpb, Bq, n, m):
    """The five outputs, every byte 0xA5."""
    out = qpb._empty_solution(Bq, n, m, torch.device("cuda"))
    for t in out:
        t.view(torch.uint8).fill_(0xA5)
    return out


def _solve_eq(qpb, H, f, A, b, meq, **kw):
    """solve_eq into outputs filled with 0xA5: every element of every output
    must have been written, whatever the status."""
    Bq, n = f.shape
    m = A.shape[1]
    sol = _host(qpb.solve_eq(*_dev(H, f, A, b), meq, out=_filled(qpb, Bq, n, m), **kw))
    for name, a in zip(("x", "lam", "active", "status", "iters"), sol):
        raw = a.view(np.int64) if a.dtype == np.float64 else a.view(np.int32)
        assert not (raw == (FILL8 if a.dtype == np.float64 else FILL4)).any(), (name, "elements never written")
    return sol


def _solve(qpb, H, f, A, b, **kw):
    return _host(qpb.solve(*_dev(H, f, A, b), **kw))


def _same(a, b):
    return all(np.array_equal(u.view(np.uint8), v.view(np.uint8)) for u, v in zip(a, b))


def _take(sol, idx):
    return [v[idx] for v in sol]


def _kkt(H, f, A, b, meq, x, lam):
    return {k: float(v.max()) for k, v in EO.kkt_mixed(H, f, A, b, meq, x, lam).items()}


def _relx(x, xr):
    return np.abs(x - xr).max(axis=1) / np.maximum(1.0, np.abs(xr).max(axis=1))


def _rell(lam, lr):
    return np.abs(lam - lr).max(axis=1) / (1.0 + np.abs(lr).max(axis=1))


# ---------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("n,m,meq", DENSE_SHAPES + WAVE_SHAPES)
def test_parity(qpb, n, m, meq):
    H, f, A, b, xc, refs = EO.eq_reference(SEED[(n, m, meq)], B, n, m, meq)
    x, lam, act, st, it = _solve_eq(qpb, H, f, A, b, meq)
    mask = qpb.active_mask_to_bool(act, m)
    xr = np.array([r.x for r in refs])
    lr = np.array([r.lam for r in refs])
    ar = np.array([r.active for r in refs])
    worst = _kkt(H, f, A, b, meq, x, lam)
    bits = mask.sum(axis=1)
    drops = int((it > bits + 1).sum())
    x0 = np.linalg.solve(H, -f[:, :, None])[:, :, 0]
    side = np.einsum("bij,bj->bi", A[:, :meq], x0) - b[:, :meq]
    print(f"({n},{m},{meq}): status {np.bincount(st, minlength=5).tolist()} x err {_relx(x, xr).max():.2e} "
          f"lam err {_rell(lam, lr).max():.2e} kkt {max(worst.values()):.2e} "
          f"mask mismatches {int((mask != ar).any(axis=1).sum())} iters {it.min()}..{it.max()} "
          f"QPs with a DROP {drops} lam_eq<0 {(lam[:, :meq] < 0).mean():.2f} a.x0<d {(side < 0).mean():.2f}")
    assert (st == OK).all(), st
    assert _relx(x, xr).max() <= X_TOL
    assert _rell(lam, lr).max() <= 1e-6
    assert np.array_equal(mask[:, meq:], ar[:, meq:])
    assert mask[:, :meq].all()
    assert all(v <= KKT_TOL for v in worst.values()), worst
    assert (it > bits).all() and (it <= 4 * (n + m) + 8).all()
    if meq < n:  # the inputs exercise the feature
        assert (lam[:, :meq] < 0).any() and (lam[:, :meq] > 0).any()
        assert (side < 0).any() and (side > 0).any()
        assert (it > bits).any()
        if n - meq >= 2:
            assert drops >= 1


# ------------------------------------------------------------- 2. meq == 0
@pytest.mark.parametrize("n,m", [(16, 32), (7, 13), (20, 33), (48, 96)])
def test_meq_zero_is_solve(qpb, n, m):
    import oracle as O
    H, f, A, b, _ = O.family_shifted(200 + n + m, 13, n, m)
    want = _solve(qpb, H, f, A, b)
    assert (want[3] == OK).all()
    assert _same(_solve_eq(qpb, H, f, A, b, 0), want)


# --------------------------------------------- 3. against the existing kernel
@pytest.mark.parametrize("n,m,meq", [(16, 26, 3), (20, 40, 4)])
def test_against_two_inequalities(qpb, n, m, meq):
    """a x = d as the pair a x <= d, -a x <= -d through qpb_solve (m + meq rows)."""
    H, f, A, b, xc = EO.eq_family(11 + n + meq, B, n, m, meq)
    x, lam, act, st, it = _solve_eq(qpb, H, f, A, b, meq)
    A2 = np.concatenate([A, -A[:, :meq]], axis=1)
    b2 = np.concatenate([b, -b[:, :meq]], axis=1)
    x2, lam2, act2, st2, it2 = _solve(qpb, H, f, A2, b2)
    assert (st == OK).all() and (st2 == OK).all(), (st, st2)
    lam_eq = lam2[:, :meq] - lam2[:, m:]
    print(f"({n},{m},{meq}): x diff {_relx(x, x2).max():.2e} lam_eq diff {_rell(lam[:, :meq], lam_eq).max():.2e} "
          f"iters eq {it.mean():.2f} pairs {it2.mean():.2f}")
    assert _relx(x, x2).max() <= X_TOL
    assert _rell(lam[:, :meq], lam_eq).max() <= 1e-6
    assert _rell(lam[:, meq:], lam2[:, meq:m]).max() <= 1e-6
    assert np.array_equal(qpb.active_mask_to_bool(act, m)[:, meq:], qpb.active_mask_to_bool(act2, m + meq)[:, meq:m])


# ------------------------------------------------------------- 4. independence
@pytest.mark.parametrize("n,m,meq", [(16, 32, 4), (20, 33, 5)])
def test_independence(qpb, n, m, meq):
    """The batch as given, permuted, and 8 of its QPs each alone: slot 1 holds
    an all-NaN QP and slot 2 an infeasible one (equality row 1 = row 0 with
    another b); every other QP's outputs are bitwise equal across the three."""
    H, f, A, b, xc = (v.copy() for v in EO.eq_reference(SEED[(n, m, meq)], B, n, m, meq)[:5])
    H[1], f[1], A[1], b[1] = np.nan, np.nan, np.nan, np.nan
    A[2, 1] = A[2, 0]
    b[2, 1] = b[2, 0] + 1.0
    base = _solve_eq(qpb, H, f, A, b, meq)
    others = np.array([i for i in range(B) if i not in (1, 2)])
    assert base[3][1] != OK and base[3][2] == INFEASIBLE, base[3][:3]
    assert (base[3][others] == OK).all()
    perm = np.random.default_rng(5).permutation(B)
    got = _solve_eq(qpb, H[perm], f[perm], A[perm], b[perm], meq)
    inv = np.argsort(perm)
    assert _same(_take(_take(got, inv), others), _take(base, others))
    for i in (0, 3, 4, 7, 21, 40, 65, 66):
        one = _solve_eq(qpb, H[i:i + 1], f[i:i + 1], A[i:i + 1], b[i:i + 1], meq)
        assert _same(one, _take(base, slice(i, i + 1))), i


# ------------------------------------------------------------ 5. status contract
CONTRACT = [(16, 32, 4), (20, 33, 4)]
CB = 16
contract = pytest.mark.parametrize("n,m,meq", CONTRACT)


def _contract_family(n, m, meq):
    return tuple(v.copy() for v in EO.eq_family(300 + n + m, CB, n, m, meq))


def _eq_bits(qpb, act, m, meq):
    return qpb.active_mask_to_bool(act, m)[:, :meq]


@contract
def test_dependent_equality(qpb, n, m, meq):
    """Equality row 3 = 2.5 x row 1.  Consistent b: OK, rank(E) = 3 equality
    bits, the row left out has lam = 0, the certificate holds and x is that of
    the QP without row 3.  b + 1: INFEASIBLE."""
    H, f, A, b, xc = _contract_family(n, m, meq)
    A[:, 3] = 2.5 * A[:, 1]
    b[:, 3] = 2.5 * b[:, 1]
    x, lam, act, st, it = _solve_eq(qpb, H, f, A, b, meq)
    assert (st == OK).all(), st
    bits = _eq_bits(qpb, act, m, meq)
    assert (bits.sum(axis=1) == 3).all() and bits[:, [0, 2]].all(), bits
    assert (lam[:, :meq][~bits] == 0).all()
    worst = _kkt(H, f, A, b, meq, x, lam)
    assert all(v <= KKT_TOL for v in worst.values()), worst
    keep = [i for i in range(m) if i != 3]
    ref = _solve_eq(qpb, H, f, A[:, keep], b[:, keep], meq - 1)
    assert (ref[3] == OK).all()
    assert _relx(x, ref[0]).max() <= X_TOL
    b[:, 3] += 1.0
    bad = _solve_eq(qpb, H, f, A, b, meq)
    assert (bad[3] == INFEASIBLE).all(), bad[3]
    assert (bad[4] >= 1).all() and np.isfinite(bad[0]).all() and np.isfinite(bad[1]).all()


@contract
def test_zero_equality_row(qpb, n, m, meq):
    """A zero equality row: b = 0 is left out (OK, 3 bits), b = 1e-3 is infeasible in the set-up."""
    H, f, A, b, xc = _contract_family(n, m, meq)
    A[:, 2] = 0.0
    b[:, 2] = 0.0
    x, lam, act, st, it = _solve_eq(qpb, H, f, A, b, meq)
    assert (st == OK).all(), st
    bits = _eq_bits(qpb, act, m, meq)
    assert (bits.sum(axis=1) == 3).all() and not bits[:, 2].any()
    assert (lam[:, 2] == 0).all()
    worst = _kkt(H, f, A, b, meq, x, lam)
    assert all(v <= KKT_TOL for v in worst.values()), worst
    for sign in (1.0, -1.0):
        b[:, 2] = sign * 1e-3
        x, lam, act, st, it = _solve_eq(qpb, H, f, A, b, meq)
        assert (st == INFEASIBLE).all(), (sign, st)
        assert (it == 0).all() and (lam == 0).all() and (act == 0).all()


@contract
def test_inequality_against_equalities(qpb, n, m, meq):
    """Inequality row 10 = equality row 0: with b - 1 it contradicts the
    equality, which is never dropped (INFEASIBLE); as -row 0 with b = -b_0 it
    is the equality's other side, tight and dependent (OK)."""
    H, f, A, b, xc = _contract_family(n, m, meq)
    A[:, 10] = A[:, 0]
    b[:, 10] = b[:, 0] - 1.0
    x, lam, act, st, it = sol = _solve_eq(qpb, H, f, A, b, meq)
    assert (st == INFEASIBLE).all(), st
    assert (it >= 1).all() and np.isfinite(x).all() and np.isfinite(lam).all()
    assert (lam[:, meq:] >= 0).all()
    A[:, 10] = -A[:, 0]
    b[:, 10] = -b[:, 0]
    x, lam, act, st, it = _solve_eq(qpb, H, f, A, b, meq)
    assert (st == OK).all(), st
    assert _eq_bits(qpb, act, m, meq).all()
    worst = _kkt(H, f, A, b, meq, x, lam)
    assert all(v <= KKT_TOL for v in worst.values()), worst


def test_more_equalities_than_variables(qpb):
    """(4, 8, 6): meq > n and consistent.  OK, rank(E) = 4 equality bits, x = xc."""
    n, m, meq = 4, 8, 6
    H, f, A, b, xc = EO.eq_family(300 + n + m, CB, n, m, meq)
    x, lam, act, st, it = _solve_eq(qpb, H, f, A, b, meq)
    assert (st == OK).all(), st
    bits = _eq_bits(qpb, act, m, meq)
    assert (bits.sum(axis=1) == 4).all()
    assert (lam[:, :meq][~bits] == 0).all()
    assert _relx(x, xc).max() <= X_TOL


@contract
def test_non_finite_b(qpb, n, m, meq):
    """NaN, +Inf, -Inf in an equality's b: NUMERICAL from the set-up.  The same
    NaN in an inequality's b still means the row is absent (as b = +inf)."""
    H, f, A, b, xc = _contract_family(n, m, meq)
    clean = _solve_eq(qpb, H, f, A, b, meq)
    assert (clean[3] == OK).all()
    for k, v in enumerate((np.nan, np.inf, -np.inf)):
        bp = b.copy()
        bp[2 * k + 1, k] = v
        x, lam, act, st, it = sol = _solve_eq(qpb, H, f, A, bp, meq)
        j = 2 * k + 1
        assert st[j] == NUMERICAL, (v, st)
        assert it[j] == 0 and (lam[j] == 0).all() and (act[j] == 0).all()
        others = np.arange(CB) != j
        assert _same(_take(sol, others), _take(clean, others)), v
    mask = qpb.active_mask_to_bool(clean[2], m)
    j = int(np.argmax(mask[:, meq:].sum(axis=1)))
    assert mask[j, meq:].any()
    r = meq + int(np.argmax(mask[j, meq:]))
    bn, bi = b.copy(), b.copy()
    bn[j, r], bi[j, r] = np.nan, np.inf
    got, want = _solve_eq(qpb, H, f, A, bn, meq), _solve_eq(qpb, H, f, A, bi, meq)
    assert (want[3] == OK).all() and not qpb.active_mask_to_bool(want[2], m)[j, r]
    assert _same(got, want)


@contract
def test_max_iter(qpb, n, m, meq):
    """max_iter = meq - 1 stops inside the equality phase: MAX_ITER, iters =
    max_iter, finite lam, stationarity.  max_iter = a QP's own uncapped iters:
    OK and bitwise the uncapped outputs."""
    H, f, A, b, xc = _contract_family(n, m, meq)
    full = _solve_eq(qpb, H, f, A, b, meq)
    assert (full[3] == OK).all()
    x, lam, act, st, it = _solve_eq(qpb, H, f, A, b, meq, max_iter=meq - 1)
    assert (st == MAX_ITER).all() and (it == meq - 1).all(), (st, it)
    assert np.isfinite(x).all() and np.isfinite(lam).all()
    mask = qpb.active_mask_to_bool(act, m)
    assert (mask.sum(axis=1) == meq - 1).all() and not mask[:, meq:].any() and (lam[~mask] == 0).all()
    assert _kkt(H, f, A, b, meq, x, lam)["stat"] <= KKT_TOL
    for K in np.unique(full[4]):
        capped = _solve_eq(qpb, H, f, A, b, meq, max_iter=int(K))
        sel = full[4] == K
        assert (capped[3][sel] == OK).all(), K
        assert _same(_take(capped, sel), _take(full, sel)), K
        assert (capped[3][full[4] > K] == MAX_ITER).all()


@contract
def test_not_spd(qpb, n, m, meq):
    H, f, A, b, xc = _contract_family(n, m, meq)
    H[1::2] *= -1.0
    x, lam, act, st, it = _solve_eq(qpb, H, f, A, b, meq)
    assert (st[1::2] == NOT_SPD).all() and (st[0::2] == OK).all(), st
    assert (it[1::2] == 0).all() and (lam[1::2] == 0).all() and (act[1::2] == 0).all()


# ------------------------------------------------------------------ 6. plumbing
@pytest.mark.parametrize("n,m,meq", [(16, 32, 4), (20, 33, 5)])
def test_plumbing(qpb, n, m, meq):
    """A side stream, the host-pointer call, iters = NULL and a batch of 1."""
    H, f, A, b, xc = EO.eq_reference(SEED[(n, m, meq)], B, n, m, meq)[:5]
    want = _solve_eq(qpb, H, f, A, b, meq)
    ins = _dev(H, f, A, b)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    sol = qpb.solve_eq(*ins, meq, stream=side)
    side.synchronize()
    assert _same(_host(sol), want)
    hs = qpb.solve_eq_host(H, f, A, b, meq)
    assert _same([np.asarray(v).view(want[k].dtype) for k, v in enumerate(hs)], want)
    out = _filled(qpb, B, n, m)
    d = qpb.Desc(n, m, B, 0, 0, 0.0)
    vp = ctypes.c_void_p
    rc = qpb.lib().qpb_solve_eq(ctypes.byref(d), meq, *[vp(t.data_ptr()) for t in ins + list(out[:4])], None,
                                vp(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    assert _same(_host(out[:4]), want[:4])
    one = _solve_eq(qpb, H[5:6], f[5:6], A[5:6], b[5:6], meq)
    assert _same(one, _take(want, slice(5, 6)))
    with pytest.raises(qpb.QPBError) as e:
        qpb.solve_eq(*_dev(*EO.eq_family(1, 2, 33, 40, 2)[:4]), 2)
    assert e.value.code == qpb.ERR_UNSUPPORTED
