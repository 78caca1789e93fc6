"""qpb_solve_backward on masks, multipliers and conditioning of the test's own.

tests/test_gpu_backward.py feeds the backward what the forward returns on one
well-conditioned family.  The backward is a function of the CALLER's active,
lam and x, so here every edge is reached directly (tests/bwd_cases.py): every
row index as the only active row, rows l and l + 16 (one lane of the n <= 16
kernel), rows 31 and 32 (the two mask words), |W| = 0 .. n from all m rows,
more than n bits, a row that is a combination of two earlier ones, weakly
active rows, bits at positions >= m, QPs that are not QPB_OK with NaN and Inf
in every input, batches of 1 to 5, power-of-two scalings, and cond(H) up to
1e10 with |W| up to n.

No reference is the code under test: closed forms (one_hot), the numpy oracle
tests/kkt_oracle.py (sizes, pairs, overfull, weak), the exact scaling law
(scaled), an mpmath solve at 50 digits (conditioned, tests/golden/bwd_cond_*).
"Bit for bit" compares two launches of the same QP.  The bars are the
project's: every array within X_TOL = 1e-6 (bwd_harness.rel), the certificate
of the outputs <= KKT_TOL = 1e-9, gH == gH^T bit for bit, exact zeros where
qpb.h says so, all outputs finite; every call checks its footprint
(bwd_harness.backward: guard words and 0xA5 fill).

Which test launches which form of qpb_kkt_bwd.hip (bwd_cases.ROUTES):

  kkt_bwd_dense_kernel<1,false>  (7, 14)            sizes one_hot overfull weak bits lockstep non_ok scaled
  kkt_bwd_dense_kernel<2,false>  (13, 26) (15, 17)  sizes one_hot pairs overfull weak bits lockstep non_ok conditioned
  kkt_bwd_dense_kernel<1,true>   (16, 16) (16, 0)   sizes one_hot overfull weak lockstep non_ok
  kkt_bwd_dense_kernel<2,true>   (16, 32)           sizes one_hot pairs overfull weak lockstep non_ok scaled conditioned
  kkt_bwd_wave_kernel, n <= 16, two words  (12, 33) sizes one_hot pairs overfull weak bits non_ok
  kkt_bwd_wave_kernel, one word  (20, 0) (20, 7) (24, 32) (17, 1)
                                                    sizes one_hot pairs overfull weak non_ok
  kkt_bwd_wave_kernel, two words (20, 33) (32, 64)  sizes one_hot pairs overfull weak bits non_ok scaled conditioned
"""
import numpy as np
import pytest

import bwd_cases as BC
import kkt_oracle as KO
from bwd_harness import KKT_TOL, NAMES, X_TOL, backward, rel, same

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

WITH_ROWS = [(n, m) for n, m in BC.ALL_ROUTES if m > 0]
WITH_PAIRS = [(n, m) for n, m in BC.ALL_ROUTES if m > 16]
NON_OK_STATUS = (1, 2, 3, 4, 100, -1)


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    return q


def _take(c, idx):
    """The QPs `idx` of a case (an index list or a slice)."""
    return BC.Case(c.H[idx], c.A[idx], c.mask[idx], c.x[idx], c.lam[idx], c.g[idx],
                   {k: v[idx] for k, v in c.ref.items()}, c.kept[idx])


def _concat(a, b):
    j = lambda u, v: np.concatenate([u, v])  # noqa: E731
    return BC.Case(j(a.H, b.H), j(a.A, b.A), j(a.mask, b.mask), j(a.x, b.x), j(a.lam, b.lam), j(a.g, b.g),
                   {k: j(a.ref[k], b.ref[k]) for k in a.ref}, j(a.kept, b.kept))


def _run(qpb, c, st=None, act=None):
    return backward(qpb, c.H, c.A, c.x, c.lam, BC.words(c.mask) if act is None else act, st, c.g)


def _names(c):
    return NAMES if c.A.shape[1] else NAMES[:2]


def _structure(c, out):
    """What holds whatever the numbers: the arrays asked for, finite, gH
    symmetric bit for bit, exact zeros outside W and in gb of a skipped row."""
    assert set(out) == set(_names(c))
    for k in out:
        assert np.isfinite(out[k]).all(), k
    assert np.array_equal(out["H"], out["H"].transpose(0, 2, 1))
    if c.A.shape[1]:
        assert (out["A"][~c.mask] == 0.0).all() and (out["b"][~c.mask] == 0.0).all()
        assert (out["b"][c.mask & ~c.kept] == 0.0).all()


def _certificates(c, out):
    gb = out["b"] if c.A.shape[1] else np.zeros((len(c.H), 0))
    return np.array([KO.certificate(c.H[i], c.A[i], c.kept[i], c.g[i], out["f"][i], gb[i]) for i in range(len(c.H))])


def _check(c, out, what):
    """Structure, parity with the case's reference, the certificate."""
    _structure(c, out)
    errs = {k: float(rel(out[k], c.ref[k]).max()) for k in _names(c)}
    cert = _certificates(c, out)
    n, m = c.H.shape[1], c.A.shape[1]
    print(f"{what} ({n},{m}) B {len(c.H)}: errors {errs} certificate stat {cert[:, 0].max():.2e} "
          f"prim {cert[:, 1].max():.2e}")
    for k, e in errs.items():
        assert e <= X_TOL, (k, e)
    assert cert.max() <= KKT_TOL, cert.max(axis=0)


# ------------------------------------------------------- 1. |W| = 0 .. n on every route
@pytest.mark.parametrize("n,m", BC.ALL_ROUTES)
def test_sizes_on_every_route(qpb, n, m):
    """|W| in {0, 1, n // 2, n - 1, n} drawn from all m rows, lam = 7 outside W
    (never read): parity with the oracle, the certificate, the footprint."""
    c = BC.sizes(n, m)
    _check(c, _run(qpb, c), "sizes")


# ------------------------------------------------------- 2. every row index, alone and in pairs
@pytest.mark.parametrize("n,m", WITH_ROWS)
def test_every_row_index_alone(qpb, n, m):
    """QP k has row k alone active: the closed form, for every k < m."""
    c = BC.one_hot(n, m)
    _check(c, _run(qpb, c), "one_hot")


@pytest.mark.parametrize("n,m", WITH_PAIRS)
def test_rows_sharing_a_lane_and_across_the_words(qpb, n, m):
    """{k, k + 16} for every k < m - 16 and {31, 32} where m > 32."""
    c = BC.pairs(n, m)
    _check(c, _run(qpb, c), "pairs")


# ------------------------------------------------------- 3. more than n bits, dependent and weak rows
@pytest.mark.parametrize("n,m", BC.FORM_ROUTES)
def test_overfull_mask(qpb, n, m):
    """All m bits set and row 5 = row 1 + 2 row 3: the rows that count are the
    oracle's; a skipped row gets gb = 0 exactly and gA = lam dx^T."""
    c = BC.overfull(n, m)
    out = _run(qpb, c)
    _check(c, out, "overfull")
    skipped = c.mask & ~c.kept
    assert skipped[:, 5].all() and (out["b"][skipped] == 0.0).all()
    want = c.lam[:, :, None] * c.ref["f"][:, None, :]
    for i in range(len(c.H)):
        assert rel(out["A"][i][skipped[i]][None], want[i][skipped[i]][None])[0] <= X_TOL, i


@pytest.mark.parametrize("n,m", BC.FORM_ROUTES)
def test_weakly_active_rows_count(qpb, n, m):
    """Bit set and lam = 0: the row is in the system, gb_i = -dlam_i != 0."""
    c = BC.weak(n, m)
    out = _run(qpb, c)
    _check(c, out, "weak")
    assert (out["b"][c.mask & (c.lam == 0.0)] != 0.0).all()


# ------------------------------------------------------- 4. bits at positions >= m
@pytest.mark.parametrize("n,m", [(7, 14), (13, 26), (12, 33), (20, 33)])
def test_bits_past_m_are_ignored(qpb, n, m):
    c = BC.sizes(n, m)
    clean = BC.words(c.mask)
    dirty = clean.view(np.uint32).copy()
    dirty[:, -1] |= np.uint32((0xFFFFFFFF << (m % 32)) & 0xFFFFFFFF)
    assert (dirty != clean.view(np.uint32)).any()
    assert same(_run(qpb, c, act=dirty.view(np.int32)), _run(qpb, c))


# ------------------------------------------------------- 5. lockstep and ragged batches, four QPs per wavefront
def _pool(n, m):
    """|W| = 0, 1, n // 2, n and an overfull QP (at m = 0: five QPs with no rows)."""
    if m == 0:
        return BC.sizes(n, m, reps=5)
    s = BC.sizes(n, m, reps=1)
    want = sorted({min(v, m) for v in (0, 1, n // 2, n)})
    pick = [int(np.flatnonzero(s.mask.sum(axis=1) == v)[0]) for v in want]
    return _concat(_take(s, pick), _take(BC.overfull(n, m, count=1), slice(0, 1)))


@pytest.mark.parametrize("n,m", BC.DENSE_ROUTES)
def test_lockstep_and_ragged_batches(qpb, n, m):
    """Four QPs share a wavefront's trip counts and its largest position.  One
    launch of 8 mixes the sizes of the pool, and over four rotations every kind
    sits in every slot of a group of four: each QP equals its own launch at
    B = 1 bit for bit.  Batches of 1 to 5 equal slices of the batch of 8."""
    pool = _pool(n, m)
    P = len(pool.H)
    alone = [_run(qpb, _take(pool, slice(i, i + 1))) for i in range(P)]
    _check(pool, {k: np.concatenate([a[k] for a in alone]) for k in alone[0]}, "pool")
    seen = set()
    for r in range(4):
        idx = np.array([(r + j) % P for j in range(8)])
        seen |= {(int(q), j % 4) for j, q in enumerate(idx)}
        batch = _take(pool, idx)
        out = _run(qpb, batch)
        for j, q in enumerate(idx):
            assert same({k: v[j:j + 1] for k, v in out.items()}, alone[q]), (r, j, q)
        if r == 0:
            for Bq in range(1, 6):
                assert same(_run(qpb, _take(batch, slice(0, Bq))), {k: v[:Bq] for k, v in out.items()}), Bq
    assert seen == {(q, s) for q in range(P) for s in range(4)}


# ------------------------------------------------------- 6. QPs that are not QPB_OK
@pytest.mark.parametrize("n,m", BC.FORM_ROUTES + [(16, 0), (20, 0)])
def test_non_ok_qps_get_exact_zeros(qpb, n, m):
    """status in {1, 2, 3, 4, 100, -1} with x, lam, gx and H full of NaN and
    +-Inf and every bit of `active` set, between OK QPs of the same wavefront:
    every output of theirs is exactly 0.0 (a select, never 0 * NaN), and the
    OK QPs equal their launch without them bit for bit."""
    c = BC.sizes(n, m, reps=-(-10 // len(BC.sizes_of(n, m))))
    Bq = len(c.H)
    st = np.zeros(Bq, np.int32)
    bad = [1, 2, 3, 5, 6, 8]
    st[bad] = NON_OK_STATUS
    H, x, lam, g = c.H.copy(), c.x.copy(), c.lam.copy(), c.g.copy()
    for j, i in enumerate(bad):
        v = (np.nan, np.inf, -np.inf)[j % 3]
        H[i], x[i], g[i] = v, v, v
        lam[i] = (np.inf, -np.inf, np.nan)[j % 3]
    act = BC.words(c.mask).view(np.uint32).copy()
    act[bad] = 0xFFFFFFFF
    out = backward(qpb, H, c.A, x, lam, act.view(np.int32), st, g)
    for k in out:
        assert (out[k][bad] == 0.0).all(), k
        assert np.isfinite(out[k]).all(), k
    good = np.flatnonzero(st == 0)
    ok = _take(c, good)
    ref = _run(qpb, ok, st=np.zeros(len(good), np.int32))
    assert same({k: v[good] for k, v in out.items()}, ref)
    _check(ok, ref, "non_ok neighbours")


# ------------------------------------------------------- 7. scalings by powers of two
@pytest.mark.parametrize("n,m", [(7, 14), (16, 32), (20, 33), (32, 64)])
def test_power_of_two_scalings(qpb, n, m):
    """H 2^+-40, rows of A 2^+-20 alternating, g 2^+-30 (and one mild scaling)
    against the unscaled oracle under the exact scaling law: the error is
    purely relative, max|delta| / max|ref| <= X_TOL per QP and array."""
    base = BC.sizes(n, m)
    for e in BC.SCALINGS:
        c = BC.scaled(base, *e)
        out = _run(qpb, c)
        _structure(c, out)
        errs = {k: float(BC.pure(out[k], c, k).max()) for k in NAMES}
        print(f"scaled ({n},{m}) 2^{e}: {errs}")
        for k, v in errs.items():
            assert v <= X_TOL, (e, k, v)


# ------------------------------------------------------- 8. cond(H) up to 1e10, |W| up to n
@pytest.mark.parametrize("n,m", BC.COND_SHAPES)
def test_ill_conditioned_h(qpb, n, m):
    """H = Q diag(logspace(0, -p)) Q^T, p in {3, 6, 10}, |W| in {0, 1, n // 2,
    n - 1, n}, against the 50-digit references of tests/golden/bwd_cond_*.npz:
    (a) the certificate <= KKT_TOL on every case;
    (b) per array, rel against the reference <= max(floor, 10 x the numpy
        oracle's own error on that case).
    The floor (bwd_cases.COND_FLOOR = 1.89e-13) is 10 x the worst error
    measured on the p = 3 cases with kkt_bwd v1.1 on an MI355X, 1.89e-14 at
    (32, 64) (1.77e-14, 1.53e-14 and 8.86e-15 at the other shapes).

    Measured on an MI355X (DESIGN.md 2.10 has the table).  kkt_bwd v1.0 missed
    (a) on all four shapes: A_W dx at p = 10 was 1.1e-6 .. 3.0e-6 with
    |W| = n and 7.4e-9 .. 2.1e-8 with |W| = n - 1 (one projection of
    u = L^-1 g), and in the four-per-wave kernel stationarity reached 4.1e-9
    as well (D = A L^-T from the other triangle of the trailing block than
    L).  kkt_bwd v1.1: certificate <= 1.4e-13 (stationarity) and <= 1.2e-15
    (A_W dx) over all 60 cases; the largest error / bar of (b) is 0.87, at
    (13, 26), p = 6, |W| = 1."""
    c, p, size, oerr = BC.conditioned_fixture(n, m)
    out = _run(qpb, c)
    _structure(c, out)
    cert = _certificates(c, out)
    err = np.stack([rel(out[k], c.ref[k]) for k in NAMES], axis=1)
    bar = np.maximum(BC.COND_FLOOR, 10.0 * oerr)
    for i in range(len(c.H)):
        print(f"cond ({n},{m}) p {p[i]} |W| {size[i]}: stat {cert[i, 0]:.2e} prim {cert[i, 1]:.2e} "
              f"errors {' '.join(f'{v:.2e}' for v in err[i])} oracle {' '.join(f'{v:.2e}' for v in oerr[i])}")
    print(f"cond ({n},{m}) worst error at p = 3: {err[p == 3].max():.2e}")
    assert cert.max() <= KKT_TOL, [(int(p[i]), int(size[i]), cert[i]) for i in np.flatnonzero(cert.max(axis=1) > KKT_TOL)]
    miss = np.argwhere(err > bar)
    assert len(miss) == 0, [(int(p[i]), int(size[i]), NAMES[j], err[i, j] / bar[i, j]) for i, j in miss]
