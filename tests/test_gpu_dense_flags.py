"""The active flags of gi_dense (csrc/qpb_gi.hip, gi_group) and the
wave-uniform bound of its back substitution, on every form of it.

A row of the active set is marked in its threshold: the high word of thr[r]
is a quiet NaN while the row is in the set (the selection's s < thr is then
false), a DROP puts the saved word back, and the active words are the
ballots of thr != thr.  The bound of the back substitution, qmax, is one
value for the four QPs of a wave, so a QP's steps depend on its wave-mates'
active sets.  What can go wrong with either:

  histories      a row added, dropped and absent at the end must lose the
                 mark; a row dropped and added again must carry it; both for
                 a row held in the lane's first register row (index < 16) and
                 in its second.  A drop cannot be planted, so the histories
                 come from the numpy model of the iteration in
                 tests/test_gpu_dense_output_phase.py (`_gi_trace`), and the
                 test first asserts them on the model.
  never active   rows that can never be selected -- a zero row of A with
                 b >= 0 (threshold -inf), b = +inf, b = NaN (an absent row),
                 the padding rows of the forms with m < 16 MR -- must never
                 show in the active word.
  an input NaN   a NaN entry of A makes a threshold NaN before any row is
                 active: that QP is QPB_NUMERICAL with an empty set, and its
                 wave-mates do not notice.
  far apart      one QP with 12 active rows beside three that end with at
                 most one: the substitution's steps above 8 run for the long
                 QP after its mates have left the loop, in each of the four
                 slots.

The planted QPs are tests/test_gpu_dense_output_phase.py's (`_planted`, from
tests/planted.py's integer parts: the final active set is unique and strictly
complementary), checked as there: the mask bit for bit, x and lam within 1e-9
relative of the dense KKT solve on the planted set (integer data, cond(H) < 12,
|x*| <= 3: five orders of margin in fp64).  The far-apart wave is also held to
tests/test_gpu_degenerate.py's bounds, x within 1e-9 of x* and the four KKT
residuals of oracle.kkt_residuals within 1e-9.
"""
import numpy as np
import pytest

import test_gpu_dense_output_phase as OP

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

X_TOL = 1e-9    # tests/test_gpu_degenerate.py
KKT_TOL = 1e-9  # tests/test_gpu_degenerate.py
OK, NUMERICAL = 0, 4


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    return q


_dev, _host, _same = OP._dev, OP._host, OP._same


# ------------------------------------------------------------------ histories
SEED_A, SEED_B = 0, 5  # seeds of OP._random_qp with the histories asserted below


@pytest.fixture(scope="module")
def histories():
    out = []
    for seed in (SEED_A, SEED_B):
        q = OP._random_qp(seed)
        trips, ev, W = OP._gi_trace(*q)
        assert W is not None, seed
        out.append((q, trips, ev, W) + OP._history(ev, W))
    return out


def test_histories(qpb, histories):
    """The model first: the two QPs show, between them, a row dropped and
    absent at the end and a row dropped and added again, each at an index
    below 16 and at one of 16 or above.  Then two waves on the GPU: the two
    QPs with planted partners of 1 and 0 active rows, and in other slots
    beside partners of 0 and 9.  The GPU takes the model's trips + 1 (the last
    finds no violated row), ends on the model's set -- the rows dropped for
    good are not in the word, those added again are -- lam is exactly 0 off
    it, and x and lam meet the KKT solve on it."""
    gone = set().union(*(h[4] for h in histories))
    back = set().union(*(h[5] for h in histories))
    print(f"dropped and absent {sorted(gone)}, dropped and added again {sorted(back)}")
    assert any(r < 16 for r in gone) and any(r >= 16 for r in gone), gone
    assert any(r < 16 for r in back) and any(r >= 16 for r in back), back
    (qa, ta, ea, Wa, _, _), (qb, tb, eb, Wb, _, _) = histories
    p1, p0, p9 = (OP._planted(16, 32, k, 1190 + k) for k in (1, 0, 9))
    order = [qa, p1[:4], qb, p0[:4], p0[:4], qb, p9[:4], qa]
    H, f, A, b = (np.stack(v) for v in zip(*order))
    tight = np.zeros((8, 32), bool)
    for i, W in ((0, Wa), (7, Wa), (2, Wb), (5, Wb)):
        tight[i, W] = True
    tight[1], tight[3], tight[4], tight[6] = p1[6], p0[6], p0[6], p9[6]
    sol = _host(qpb.solve(*_dev(H, f, A, b)))
    print(f"model A: {ea}\nmodel B: {eb}")
    OP._check(qpb, sol, H, f, A, b, tight, "histories")
    mask = qpb.active_mask_to_bool(sol[2], 32)
    assert (sol[1][~mask] == 0.0).all()
    assert sol[4][[0, 7]].tolist() == [ta + 1] * 2 and sol[4][[2, 5]].tolist() == [tb + 1] * 2, (sol[4], ta, tb)


# ------------------------------------------------- rows that are never active
def _never(row):
    """A wave of planted QPs with 9, 3, 12 and 0 active rows in which the first
    three rows from `row` on that are not tight (they keep an integer slack
    >= 1 at x*, so the solution does not depend on them) become a zero row
    with b = 2, a row with b = +inf and a row with b = NaN; all three stay in
    `row`'s half of the 32 rows."""
    H, f, A, b, xs, _, tight = OP._batch(16, 32, [9, 3, 12, 0], 1200 + row)
    for i in range(4):
        z, pinf, pnan = [r for r in range(row, 32) if not tight[i, r]][:3]
        assert pnan // 16 == row // 16, (i, pnan)
        A[i, z], b[i, z] = 0.0, 2.0
        b[i, pinf] = np.inf
        b[i, pnan] = np.nan
    return H, f, A, b, xs, tight


@pytest.mark.parametrize("row", [3, 19])
def test_rows_never_active(qpb, row):
    """The three kinds of row that no trip can select, at indices from `row`
    on (below 16: the lane's first register row; 16 or above: its second)."""
    H, f, A, b, xs, tight = _never(row)
    assert (np.isinf(b).sum(axis=1) == 1).all() and (np.isnan(b).sum(axis=1) == 1).all()
    sol = _host(qpb.solve(*_dev(H, f, A, b)))
    OP._check(qpb, sol, H, f, A, b, tight, f"never active from row {row}")
    assert np.abs(sol[0] - xs).max() <= 3.0 * X_TOL  # the planted x*, |x*| <= 3


@pytest.mark.parametrize("n,m", [(16, 20), (16, 9), (7, 11)])
def test_padding_rows_never_active(qpb, n, m):
    """m < 16 MR: the rows from m up to 16 or 32 exist only in the lanes.  No
    bit at or above m is ever set in the word, and the mask is the planted
    one, with sets from empty up to min(n, m) rows."""
    top = min(n, m)
    sizes = [top, 0, 1, top - 1, 2]
    H, f, A, b, _, _, tight = OP._batch(n, m, sizes, 1210)
    sol = _host(qpb.solve(*_dev(H, f, A, b)))
    OP._check(qpb, sol, H, f, A, b, tight, f"padding n={n} m={m}")
    word = sol[2].astype(np.int64).reshape(len(sizes), -1)[:, 0] & 0xFFFFFFFF
    assert (word >> m == 0).all(), [hex(w) for w in word]


# ---------------------------------------------------------- a NaN entry in A
@pytest.mark.parametrize("row", [5, 21])
def test_nan_entry_in_a(qpb, row):
    """QP 1 of the wave has a NaN in row `row` of A: QPB_NUMERICAL, no trip,
    an empty set and lam = 0 (the row's NaN threshold is no active mark).  Its
    three wave-mates are bit for bit what they are when solved alone."""
    H, f, A, b, _, _, tight = OP._batch(16, 32, [9, 9, 1, 12], 1220)
    A[1, row, 7] = np.nan
    sol = _host(qpb.solve(*_dev(H, f, A, b)))
    x, lam, act, st, it = sol
    assert st.tolist() == [OK, NUMERICAL, OK, OK], st
    assert it[1] == 0 and (lam[1] == 0.0).all() and not qpb.active_mask_to_bool(act, 32)[1].any()
    keep = [0, 2, 3]
    for i in keep:
        alone = _host(qpb.solve(*_dev(H[i:i + 1], f[i:i + 1], A[i:i + 1], b[i:i + 1])))
        assert _same([v[i:i + 1] for v in sol], alone), i
    OP._check(qpb, [v[keep] for v in sol], H[keep], f[keep], A[keep], b[keep], tight[keep], "mates of a NaN QP")


# ----------------------------------------------- a wave whose rows end far apart
LONG, MATES = 12, [0, 1, 1]


def _far_apart(slot):
    sizes = MATES[:slot] + [LONG] + MATES[slot:]
    return OP._batch(16, 32, sizes, 1230 + slot)


def _degenerate_bounds(H, f, A, b, xs, sol, what):
    """tests/test_gpu_degenerate.py's: x within 1e-9 relative of x*, the four
    KKT residuals of the GPU's own answer within 1e-9."""
    import oracle as O
    ex = np.abs(sol[0] - xs).max(axis=1) / np.maximum(1.0, np.abs(xs).max(axis=1))
    worst = {k: float(v.max()) for k, v in O.kkt_residuals(H, f, A, b, sol[0], sol[1]).items()}
    print(f"{what}: x err {ex.max():.2e}, kkt {worst}")
    assert ex.max() <= X_TOL, (what, ex)
    assert all(v <= KKT_TOL for v in worst.values()), (what, worst)


@pytest.mark.parametrize("slot", [0, 1, 2, 3])
def test_rows_end_far_apart(qpb, slot):
    """The long QP (12 active rows: substitution steps up to column 11) in
    slot `slot`, its mates ending with at most one row."""
    H, f, A, b, xs, _, tight = _far_apart(slot)
    assert tight.sum(axis=1).tolist() == MATES[:slot] + [LONG] + MATES[slot:]
    sol = _host(qpb.solve(*_dev(H, f, A, b)))
    OP._check(qpb, sol, H, f, A, b, tight, f"far apart, slot {slot}")
    _degenerate_bounds(H, f, A, b, xs, sol, f"far apart, slot {slot}")
    assert sol[4][slot] >= LONG + 1 and (np.delete(sol[4], slot) < sol[4][slot]).all(), sol[4]


def test_rows_end_far_apart_ragged(qpb):
    """A batch of 5: the second wave holds the long QP alone, beside three
    rows that replay it and store nothing."""
    qs = [OP._planted(16, 32, k, 1240 + i) for i, k in enumerate([1, LONG, 0, 1, LONG])]
    H, f, A, b, xs, _, tight = (np.stack(v) for v in zip(*qs))
    sol = _host(qpb.solve(*_dev(H, f, A, b)))
    OP._check(qpb, sol, H, f, A, b, tight, "far apart, ragged")
    _degenerate_bounds(H, f, A, b, xs, sol, "far apart, ragged")


# ------------------------------------------------- the other forms of gi_group
SIZES = MATES[:1] + [LONG] + MATES[1:] + [9]  # a far-apart wave and a wave of one


def test_eq_form(qpb):
    """qpb_solve_eq, meq = 2: the equalities hold positions 0 and 1, so the
    long QP ends with 14 rows."""
    H, f, A, b, _, _, tight = OP._batch(16, 32, SIZES, 1250, meq=2)
    sol = _host(qpb.solve_eq(*_dev(H, f, A, b), 2))
    OP._check(qpb, sol, H, f, A, b, tight, "eq", meq=2)
    assert qpb.active_mask_to_bool(sol[2], 32)[:, :2].all()


def test_range_form(qpb):
    """qpb_solve_range, as tests/test_gpu_dense_output_phase.py builds it: the
    tight rows at odd indices are held at their lower side; the `lower` word
    marks exactly them."""
    H, f, A, b, _, _, tight = OP._batch(16, 32, SIZES, 1251)
    odd = (np.arange(32) % 2 == 1)[None, :]
    low = tight & odd
    A2 = np.where(low[:, :, None], -A, A)
    bu = np.where(low, np.where(np.arange(32) % 4 == 1, np.inf, -b + 7.0), b)
    bl = np.where(low, -b, b - 20.0)
    rhs = np.where(low, bl, bu)
    sol = _host(qpb.solve_range(*_dev(H, f, A2, bl, bu)))
    OP._check(qpb, sol, H, f, A2, rhs, tight, "range", signed=True)
    assert np.array_equal(qpb.active_mask_to_bool(sol[3], 32), low)
    assert (sol[1][low] < 0.0).all() and (sol[1][tight & ~low] > 0.0).all()


def test_shared_and_factored_forms(qpb):
    """qpb_solve_shared on one H and one A: bitwise qpb_solve on copies, and
    the planted sets.  qpb_solve_factored on the same case: the shared solve's
    status and words, x and lam within the tolerance."""
    H, A, f, b, tight = OP._shared_case(1252, SIZES)
    B = len(SIZES)
    Ht, At = np.broadcast_to(H, (B, 16, 16)).copy(), np.broadcast_to(A, (B, 32, 16)).copy()
    plain = _host(qpb.solve(*_dev(Ht, f, At, b)))
    Hd, Ad, fd, bd = _dev(H, A, f, b)
    shared = _host(qpb.solve_shared(Hd, fd, Ad, bd))
    assert _same(shared, plain)
    OP._check(qpb, shared, H, f, A, b, tight, "shared")
    F = qpb.factor_shared(Hd, Ad)
    fact = _host(qpb.solve_factored(F, fd, bd))
    assert int(F.status.cpu()[0]) == OK
    OP._check(qpb, fact, H, f, A, b, tight, "factored")
    assert np.array_equal(fact[2], shared[2]) and np.array_equal(fact[3], shared[3])
