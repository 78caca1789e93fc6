"""The n <= 16 kernel runs four QPs per wavefront in lockstep and takes
wave-uniform shortcuts (bounds over the four rows' active-set sizes, trips
that only some rows need).  None of them may leak from one QP into another:

  1. a QP's outputs do not depend on its wave-mates (a mixed launch against
     every QP alone, bitwise);
  2. nor on its slot in the wave or on ragged replay rows (all 24 orders of one
     wave; B = 1, 2, 3, 5, 7);
  3. the same for the other instantiations (MR = 1, not FULL, padded n), each
     against the oracle as well;
  4. the bench families' outputs are bitwise those of gi_dense v11.5
     (tests/golden/gi_dense_v115_*.npz, recorded by tools/record_dense_golden.py:
     tests/golden/gi_dense_v115.json says how);
  5. (CPU) tools/loop_account.py's lockstep replay reproduces the kernel's
     iteration and trip counts.

The QPs are chosen on the CPU with the numpy model of the kernel's iteration
(tools/gi_select_sim.py): one that needs no iteration, one that ends with all
16 positions active (q reaches the lane count), ones that drop a constraint,
and plain bench-family ones.  Batches stay <= 64 QPs.
"""
import itertools
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

X_TOL = 1e-6  # tests/test_gpu_active_set.py's oracle tolerance: x and lambda relative, masks exact
SEED = 20261015
FIELDS = ("x", "lam", "active", "status", "iters")


@pytest.fixture(scope="module")
def qpb():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    return q


def _solve(qpb, H, f, A, b):
    import torch
    dev = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda() for a in (H, f, A, b)]
    sol = qpb.solve(*dev)
    torch.cuda.synchronize()
    return [np.ascontiguousarray(t.cpu().numpy()) for t in sol]


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(
        np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _sim(H, f, A, b):
    """(iterations, drops, final active set) of the numpy model of the kernel's iteration."""
    from gi_select_sim import gi
    it, adds, drops, W = gi(H, f, A, b, "proj")
    return it, drops, W


def _zero_iteration(H, f, A, b):
    """The same QP with b so large that the unconstrained minimiser is feasible."""
    return H, f, A, np.full_like(b, 1e9)


def _all_active(H, f):
    """A box so small around 0 that every component of x0 = -H^{-1} f lies outside it and the
    gradient keeps f's signs over the whole box: all 16 bounds end active."""
    n = len(f)
    x0 = np.linalg.solve(H, -f)
    w = 1e-3 * min(np.abs(x0).min(), np.abs(f).min() / np.abs(H).sum(axis=1).max())
    return H, f, np.concatenate([np.eye(n), -np.eye(n)]), np.full(2 * n, w)


@pytest.fixture(scope="module")
def mixed():
    """<= 64 QPs at n = 16, m = 32: index 0 needs no iteration, 1 ends with 16 active rows,
    `drops` drop a constraint on the way, the rest are plain bench-family QPs."""
    import oracle as O
    n = 16
    box = O.family_generate(n, 24, SEED, family="box")
    den = O.family_generate(n, 96, SEED, family="dense")
    qps = [_zero_iteration(*(a[0] for a in box)), _all_active(box[0][1], box[1][1])]
    assert _sim(*qps[0])[0] == 0
    it, _, W = _sim(*qps[1])
    assert W is not None and len(W) == n and it >= n, (it, W)
    dropping = [i for i in range(96) if _sim(*(a[i] for a in den))[1] > 0][:6]
    assert len(dropping) >= 2, dropping
    drops = list(range(len(qps), len(qps) + len(dropping)))
    qps += [tuple(a[i] for a in den) for i in dropping]
    plain = list(range(len(qps), len(qps) + 22))
    qps += [tuple(a[i] for a in box) for i in range(2, 14)] + [tuple(a[i] for a in den) for i in range(10)]
    assert len(plain) == len(qps) - plain[0] and len(qps) <= 64
    H, f, A, b = (np.stack([q[k] for q in qps]) for k in range(4))
    return {"H": H, "f": f, "A": A, "b": b, "zero": 0, "full": 1, "drops": drops, "plain": plain}


@pytest.fixture(scope="module")
def alone(qpb, mixed):
    """Every QP of the mixed set solved by itself (B = 1): the reference of tests 1 and 2."""
    return [_solve(qpb, *(mixed[k][i:i + 1] for k in ("H", "f", "A", "b"))) for i in range(len(mixed["f"]))]


def _assert_matches_alone(out, alone, ids, what):
    for pos, i in enumerate(ids):
        for k, name in enumerate(FIELDS):
            assert _same_bits(out[k][pos:pos + 1], alone[i][k]), (what, "QP", i, "at", pos, name)


@pytest.mark.gpu
def test_answer_does_not_depend_on_wave_mates(qpb, mixed, alone):
    out = _solve(qpb, mixed["H"], mixed["f"], mixed["A"], mixed["b"])
    x, lam, act, st, it = out
    assert (st == qpb.OK).all(), st
    nact = qpb.active_mask_to_bool(act, 32).sum(axis=1)
    # the three kinds are really there (the kernel counts the last, empty selection as a trip)
    assert it[mixed["zero"]] == 1 and nact[mixed["zero"]] == 0
    assert nact[mixed["full"]] == 16
    assert all(it[i] > nact[i] + 1 for i in mixed["drops"]), (it, nact)
    _assert_matches_alone(out, alone, range(len(st)), "mixed launch")


@pytest.mark.gpu
def test_slot_permutations_and_ragged_batches(qpb, mixed, alone):
    four = [mixed["zero"], mixed["full"], mixed["drops"][0], mixed["plain"][0]]
    sel = lambda ids: [mixed[k][list(ids)] for k in ("H", "f", "A", "b")]  # noqa: E731
    for order in itertools.permutations(four):
        _assert_matches_alone(_solve(qpb, *sel(order)), alone, order, f"order {order}")
    seven = four + [mixed["drops"][1], mixed["plain"][1], mixed["plain"][2]]
    for B in (1, 2, 3, 5, 7):
        # the last wave holds B mod 4 live rows: the others replay the last QP
        for ids in (seven[:B], seven[::-1][:B]):
            _assert_matches_alone(_solve(qpb, *sel(ids)), alone, ids, f"B = {B}")


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", [(16, 16), (16, 20), (10, 20), (4, 8)])
def test_other_instantiations(qpb, n, m):
    """MR = 1 FULL, MR = 2 not FULL, and the padded forms (q <= n < 16): wave-mates and the oracle."""
    import oracle as O
    H, f, A, b = O.family_generate(n, 22, SEED + n + m, family="dense", m=m)
    # a QP that needs no iteration and, where the shape allows (m >= 2 n), one with n active bounds
    b[0] = 1e9
    if m >= 2 * n:
        _, _, A[1], b[1] = _all_active(H[1], f[1])
    out = _solve(qpb, H, f, A, b)
    x, lam, act, st, it = out
    assert (st == qpb.OK).all(), st
    mask = qpb.active_mask_to_bool(act, m)
    assert it[0] == 1 and (m < 2 * n or mask[1].sum() == n)
    assert (mask.sum(axis=1) >= 2).any()  # rows of one wave at different active-set sizes
    for i in range(len(f)):
        one = _solve(qpb, H[i:i + 1], f[i:i + 1], A[i:i + 1], b[i:i + 1])
        for k, name in enumerate(FIELDS):
            assert _same_bits(out[k][i:i + 1], one[k]), (n, m, i, name)
        ref = O.active_set_solve(H[i], f[i], A[i], b[i])
        assert ref.status == 0, i
        assert np.abs(x[i] - ref.x).max() / max(1.0, np.abs(ref.x).max()) <= X_TOL, i
        assert np.abs(lam[i] - ref.lam).max() / (1.0 + np.abs(ref.lam).max()) <= X_TOL, i
        assert np.array_equal(mask[i], ref.active), i


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["box", "dense"])
def test_results_stay_what_gi_dense_v115_gave(qpb, family):
    import torch
    g = np.load(os.path.join(GOLDEN, f"gi_dense_v115_{family}.npz"))
    H, f, A, b = qpb.generate(16, len(g["status"]), SEED, family=family, shift=1.0, box=10.0,
                              device=torch.device("cuda", 0))
    sol = qpb.solve(H, f, A, b)
    torch.cuda.synchronize()
    for name in FIELDS:
        got = getattr(sol, name).cpu().numpy()
        assert _same_bits(got, g[name]), (family, name, int((got != g[name]).sum()))


def test_lockstep_replay_reproduces_the_kernels_trip_counts():
    """tools/loop_account.py's replay on 2 000 box QPs: 4.66 iterations per QP and 7.4 trips per
    wave, the counts the kernel reports on the bench family."""
    import loop_account
    _, stats = loop_account.replay(loop_account.traces(2000, "box"))
    assert abs(stats["iterations_per_qp"] - 4.66) <= 0.05, stats
    assert abs(stats["trips_per_wave"] - 7.4) <= 0.1, stats
    assert stats["work_trips_per_wave"] == pytest.approx(stats["trips_per_wave"] - 1.0)
