"""Degenerate QPs on the two-sided routes: qpb_solve_range (the RG forms of
gi_dense and gi_wave, per QP and with a shared H and / or A), qpb_solve_range_box
(the BX forms) and qpb_solve_range_factored.

The other range tests draw non-degenerate families and compare active sets bit
for bit with an oracle.  Here the inputs are tests/planted.py's planted range
families: weakly active rows on either side, a row given again negated (the
same half-space held in the other orientation) and doubled, a vertex with more
tight rows than n - meq, a zero-width row given twice, a G row that duplicates
a variable bound, and `thin` rows whose other bound is 2^-20 away.  The
CPU test tests/test_planted.py shows that in every batch (the range-box ones
too, there among the variable bounds as well, whose other bound is 2^-20 away;
and in the first six QPs that are solved one at a time) rows are tight on the
side opposite to the one violated at the unconstrained minimiser: a kernel that
holds one side of a row at a time must flip them, or DROP them and take them
back on the other side, at a vertex with dependent rows or zero multipliers.

The active set is not unique at such a vertex, so the assertions are
tests/range_planted_checks.py's (status OK and the iteration bound on every QP,
x within 1e-9 of the planted x*, the two-sided KKT certificate <= 1e-9, `lower`
and the sign of lam consistent with the side a row is tight on, no slack row
active, A^T lam == A^T lam*, lam == lam* where it is unique, a row of every
dependent group active, `thin` bit for bit).  QP i of a launch has kind
i mod 4 with its own seed, so partners in a wavefront differ.  Each test prints
and asserts > 0 the number of its QPs with tight rows beyond the set bits.

Measured on the MI355X (measurements, not bars; worst x err / KKT residual /
A^T lam err relative, then the QPs of the launch with tight rows beyond the set
bits).  No test here needed a kernel change.

  qpb_solve_range        (7,14,2)   5.5e-15 / 9.0e-16 / 1.4e-14   37 of 37
                         (13,26,3)  3.7e-15 / 5.7e-16 / 5.4e-15   37 of 37
                         (16,16,0)  4.6e-15 / 6.4e-16 / 7.7e-15   37 of 37
                         (16,32,4)  7.3e-15 / 1.2e-15 / 1.1e-14   37 of 37
                         (16,33,0)  1.0e-15 / 1.7e-16 / 3.3e-15   13 of 13
                         (20,33,5)  1.5e-15 / 2.0e-16 / 3.5e-15   13 of 13
                         (32,64,8)  1.6e-15 / 1.8e-16 / 6.5e-15   13 of 13
    thin, all routes     <= 5.5e-15 / 6.8e-16 / 9.2e-15           0 of 3 (not degenerate)
    pair form, solve_eq  x of the two calls within 7.1e-15; iters differ on a few QPs only
  qpb_solve_range_box    (7,7,0)    6.0e-15 / 8.4e-16 / 2.0e-14   37 of 37
                         (12,20,3)  3.7e-15 / 5.9e-16 / 8.6e-15   37 of 37
                         (16,16,2)  9.5e-15 / 9.7e-16 / 2.3e-14   37 of 37
                         (16,0,0)   4.0e-15 / 1.1e-15 / 7.0e-14   13 of 13
                         (16,17,1)  1.2e-15 / 1.6e-16 / 5.1e-15   13 of 13
                         (20,9,0)   2.1e-15 / 2.3e-16 / 3.4e-14   13 of 13
                         (32,32,3)  2.1e-15 / 2.0e-16 / 1.7e-14   13 of 13
                         (32,0,0)   1.8e-15 / 4.4e-16 / 5.9e-14   13 of 13
    a pinned variable's multiplier: within 3.7e-14 of mu_j
  shared H and A         (16,32,4)  7.6e-15 / 6.7e-16 / 1.5e-14   9 of 13 (the thin QPs are not)
                         (20,33,5)  2.1e-15 / 2.4e-16 / 3.8e-15   9 of 13
  qpb_solve_range_factored, the shared batches
                         (16,32,4)  3.1e-15 / 6.4e-16 / 7.1e-15   9 of 13
                         (20,33,5)  1.9e-15 / 3.6e-16 / 4.3e-15   9 of 13
    one QP at a time, all routes    <= 5.2e-15 / 1.3e-15 / 5.3e-15   6 of 6
"""
import numpy as np
import pytest

import planted as P
import range_box_oracle as BO
import range_oracle as RO
import range_planted_checks as C

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

X_TOL = C.X_TOL
OK = 0
NAMES = ("x", "lam", "active", "lower", "status", "iters")

range_routes = pytest.mark.parametrize("n,m,meq,B", P.RANGE)
box_routes = pytest.mark.parametrize("n,mg,meq,B", P.RANGE_BOX)
shared_routes = pytest.mark.parametrize("n,m,meq,B", P.RANGE_SHARED)


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


def _range(qpb, q, meq, H=None, A=None):
    return _host(qpb.solve_range(*_dev(q.H if H is None else H, q.f, q.A if A is None else A, q.bl, q.bu), meq))


def _same(a, b):
    """Bit for bit: x and lam as bytes, so that -0.0 is not 0.0."""
    bad = [name for name, u, v in zip(NAMES, a, b)
           if u.shape != v.shape or not np.array_equal(u.view(np.uint8), v.view(np.uint8))]
    assert not bad, bad


def _thin(n, m, meq):
    return P.range_batch(n, m, meq, 3, kinds=("thin",))


# ---------------------------------------------------------- qpb_solve_range
@range_routes
def test_degenerate_range(qpb, n, m, meq, B):
    """weak / dup / vertex / pinned interleaved on every RG route."""
    q, kinds = P.range_batch(n, m, meq, B)
    r = C.check(q, kinds, _range(qpb, q, meq), f"range ({n},{m},{meq})", meq)
    assert r["degenerate"] > 0


@range_routes
def test_thin_range(qpb, n, m, meq, B):
    """Three QPs whose tight rows have the other bound 2^-20 away: not
    degenerate, so `active` and `lower` are bit-exact (the checker's thin rule)
    and lam is lam* within 1e-9."""
    q, kinds = _thin(n, m, meq)
    sol = _range(qpb, q, meq)
    C.check(q, kinds, sol, f"range ({n},{m},{meq}) thin", meq)
    assert np.abs(sol[1] - q.lam).max() <= X_TOL * (1.0 + np.abs(q.lam).max())


@pytest.mark.parametrize("n,m,meq,B", [r for r in P.RANGE if 2 * r[1] - r[2] <= 64])
def test_pair_form_through_solve_eq(qpb, n, m, meq, B):
    """The same QPs through qpb_solve_eq on the pair form [E; G; -G] (the EQ
    forms, which tests/test_gpu_degenerate.py covers): both answers meet the
    bars and x agrees within 1e-9.  The pair form's answer is mapped back with
    range_oracle.from_pairs (a zero-width row is two dependent rows there and
    may be held from both sides: the checker lets it carry either bit)."""
    q, kinds = P.range_batch(n, m, meq, B)
    t, tk = _thin(n, m, meq)
    for what, (b, ks) in (("degenerate", (q, kinds)), ("thin", (t, tk))):
        rg = _range(qpb, b, meq)
        C.check(b, ks, rg, f"range ({n},{m},{meq}) {what}", meq)
        A2, b2 = RO.to_pairs(b.A, b.bl, b.bu, meq)
        x2, lam2, act2, st2, it2 = _host(qpb.solve_eq(*_dev(b.H, b.f, A2, b2), meq))
        assert (st2 == OK).all(), st2
        mask2 = qpb.active_mask_to_bool(act2, 2 * m - meq)
        back = [RO.from_pairs(lam2[i], mask2[i], m, meq) for i in range(len(x2))]
        lam = np.array([v[0] for v in back])
        act = np.array([v[1] for v in back])
        low = np.array([v[2] for v in back])
        eq = [x2, lam, RO.pack_bits(act), RO.pack_bits(low), st2, it2]
        C.check(b, ks, eq, f"pairs ({n},{2 * m - meq},{meq}) {what}", meq)
        diff = C.relx(rg[0], x2).max()
        print(f"({n},{m},{meq}) {what}: x range vs pairs {diff:.2e}; iters {rg[5].mean():.2f} range, "
              f"{it2.mean():.2f} pairs")
        assert diff <= X_TOL


# ------------------------------------------------------ qpb_solve_range_box
@box_routes
def test_degenerate_range_box(qpb, n, mg, meq, B):
    """weak / pinned / vertex / dup_bound interleaved on every BX route: the
    checker on the materialised fields, every output bit for bit
    qpb_solve_range's on the materialised [G; I] (the call's contract, at a
    degenerate vertex too), and a pinned variable on its bound with the
    planted signed multiplier."""
    b, kinds = P.range_box_batch(n, mg, meq, B)
    G, bl, bu = (b.G, b.bl, b.bu) if mg else (None, None, None)
    box = _host(qpb.solve_range_box(*_dev(b.H, b.f, G, bl, bu, b.lb, b.ub), meq))
    q = b.materialised()
    A, lo, hi = BO.materialise(b.G, b.bl, b.bu, b.lb, b.ub, n)
    assert np.array_equal(A, q.A) and np.array_equal(lo, q.bl) and np.array_equal(hi, q.bu)
    r = C.check(q, kinds, box, f"range_box ({n},{mg},{meq})", meq)
    assert r["degenerate"] > 0
    _same(box, _range(qpb, q, meq))
    x, lam = box[0], box[1]
    assert (np.abs(x - b.lb)[b.pinned] <= X_TOL * np.maximum(1.0, np.abs(b.lb[b.pinned]))).all()
    err = np.abs(lam[:, mg:] - b.mu)[b.pinned] / (1.0 + np.abs(b.mu).max())
    print(f"range_box ({n},{mg},{meq}): pinned {int(b.pinned.sum())} mu<0 {int((b.mu[b.pinned] < 0).sum())} "
          f"mu>0 {int((b.mu[b.pinned] > 0).sum())} mu err {err.max():.2e}")
    assert b.pinned.any() and err.max() <= X_TOL


# -------------------------------------------------- shared H / A, factored
@shared_routes
def test_degenerate_range_shared(qpb, n, m, meq, B):
    """weak / vertex / thin with one H and one A: the SH forms with a 2-D H, a
    2-D A and both are bit for bit the call on copies, and the checker passes."""
    q, kinds = P.range_shared_batch(n, m, meq, B)
    want = _range(qpb, q, meq)
    r = C.check(q, kinds, want, f"range shared ({n},{m},{meq})", meq)
    assert r["degenerate"] > 0
    for Hs, As in ((q.H[0], None), (None, q.A[0]), (q.H[0], q.A[0])):
        _same(_range(qpb, q, meq, H=Hs, A=As), want)


def _factored(qpb, H0, A0, f, bl, bu, meq):
    F = qpb.factor_shared(*_dev(H0, A0))
    sol = _host(qpb.solve_range_factored(F, *_dev(f, bl, bu), meq))
    return sol, int(F.status.cpu().numpy()[0])


@shared_routes
def test_degenerate_range_factored(qpb, n, m, meq, B):
    """The shared batches from a factor buffer: the checker passes on all, and
    on the non-degenerate `thin` QPs status, `active` and `lower` equal the
    unfactored call's."""
    q, kinds = P.range_shared_batch(n, m, meq, B)
    got, fstatus = _factored(qpb, q.H[0], q.A[0], q.f, q.bl, q.bu, meq)
    assert fstatus == OK
    r = C.check(q, kinds, got, f"range factored ({n},{m},{meq})", meq)
    assert r["degenerate"] > 0
    ref = _range(qpb, q, meq, H=q.H[0], A=q.A[0])
    thin = np.array([k == "thin" for k in kinds])
    assert thin.any()
    for k in (2, 3, 4):  # active, lower, status
        assert np.array_equal(got[k][thin], ref[k][thin]), NAMES[k]


@range_routes
def test_degenerate_range_factored_one_qp_at_a_time(qpb, n, m, meq, B):
    """The first six QPs of every RANGE route's per-QP batch, each factored and
    solved as a batch of one (a single QP is a shared problem)."""
    q, kinds = P.range_batch(n, m, meq, 6)
    sols = []
    for i in range(len(kinds)):
        got, fstatus = _factored(qpb, q.H[i], q.A[i], q.f[i:i + 1], q.bl[i:i + 1], q.bu[i:i + 1], meq)
        assert fstatus == OK, (i, kinds[i], fstatus)
        sols.append(got)
    sol = [np.concatenate([s[k] for s in sols]) for k in range(6)]
    r = C.check(q, kinds, sol, f"range factored one at a time ({n},{m},{meq})", meq)
    assert r["degenerate"] > 0
