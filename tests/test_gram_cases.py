"""The conditions that make tests/test_gpu_gram_large_sets.py's inputs worth
running, asserted on the CPU (numpy only; nothing is compiled, no GPU):

  the two seams of csrc/qpb_gi_gram.hip (64 lanes, QL = 70 Q1 rows in LDS) as
    gram_cases.py states them, recomputed from the constants in the .hip file;
    if the LDS layout moves, the shapes of the GPU tests must be revisited, and
    this is the test that says so
  strict   the numpy model of the kernel's method (tools/gi_select_sim.py) ends
           on the planted set and reaches q >= k - 1
  vertex   the oracle certifies every QP and agrees with the model on the set;
           the model's DROPs fall on every seam; the multipliers and slacks
           are far enough from zero for a bit-exact mask to be a fair demand
  box      the number of QPs with more than QL active bounds

and that the constants at the end of gram_cases.py, which the GPU tests read,
are what the model and the oracle give.
"""
import functools
import os
import re

import numpy as np
import pytest

import gram_cases as G
import oracle as O

HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "embedded-qp-solver_amd", "csrc",
                   "qpb_gi_gram.hip")
MARGIN = 1e-3  # the smallest active multiplier and inactive slack a bit-exact mask may be asked at


def test_seams_follow_the_kernel_source():
    src = open(HIP).read()

    def const(name):
        return int(re.search(rf"constexpr int {name} = (\d+);", src).group(1))

    NB, NT, LDS_D, NBUF, QS = (const(k) for k in ("NB", "NT", "LDS_D", "NBUF", "QS"))
    assert re.search(r"constexpr int LP = NB \* \(NB \+ 1\) / 2;\s*// packed triangle, 8256 doubles", src)
    assert re.search(r"constexpr int OFF_ROWS = LP;", src) and re.search(r"constexpr int OFF_BUF = LDS_D - NBUF;", src)
    assert re.search(r"constexpr int QL = \(OFF_BUF - OFF_ROWS\) / QS;", src)
    LP = NB * (NB + 1) // 2
    assert (LP, LDS_D, NBUF, QS) == (8256, 20480, 2136, 144)
    assert (LDS_D - NBUF - LP) // QS == 70 == G.QL
    assert NT // 8 == 64 == G.WAVE  # 8 wavefronts: `l + 64` is a lane's second position
    assert (G.NT, G.NB, G.LDS_D, G.NBUF, G.QS, G.LP) == (NT, NB, LDS_D, NBUF, QS, LP)
    # the shapes were chosen around these two numbers
    assert {k for _, _, k in G.STRICT} >= {G.WAVE + 1, G.QL, G.QL + 1, G.QL + 2, 128}


def test_mask_hex_round_trip():
    rs = np.random.default_rng(0)
    for m in (66, 200, 256):
        mask = rs.random(m) < 0.5
        assert np.array_equal(G.hex_mask(G.mask_hex(mask), m), mask)


# ------------------------------------------------------------------- strict
@pytest.mark.parametrize("n,m,k", G.STRICT)
def test_strict_reaches_its_set(n, m, k):
    trips = []
    for seed in G.STRICT_SEEDS:
        q = G.strict_dense(n, m, k, seed)
        assert q.tight.sum() == k and (q.lam[q.tight] >= 1).all() and (q.lam[~q.tight] == 0).all()
        s = q.b - q.A @ q.x
        assert (s[q.tight] == 0).all() and (s[~q.tight] >= 1).all()
        assert np.abs(q.H @ q.x + q.f + q.A.T @ q.lam).max() == 0.0  # integer data: exact
        assert np.linalg.matrix_rank(q.A[q.tight]) == k and np.linalg.cond(q.H) < 12
        pf = G.path_facts(q.H, q.f, q.A, q.b)
        print(f"strict ({n},{m},{k}) seed {seed}: trips {pf.trips} DROPs {pf.drops} largest q {pf.max_q}")
        assert pf.final == tuple(np.nonzero(q.tight)[0])
        assert pf.max_q >= k - 1
        assert pf.add_q >= set(range(k))  # an ADD at every size below k: every loop tail is swept
        assert pf.trips + 1 <= G.iteration_cap(n, m)
        trips.append(pf.trips)
    assert tuple(trips) == G.STRICT_MODEL_TRIPS[(n, m, k)]


def test_second_qp_cases():
    n, m = G.SECOND_SHAPE
    (H, f, A, b), planted = G.second_qp_cases()
    assert H.shape == (6, n, n) and A.shape == (6, m, n)
    for name, q in planted.items():
        pf = G.path_facts(q.H, q.f, q.A, q.b)
        assert pf.final == tuple(np.nonzero(q.tight)[0]), name
        assert pf.trips == G.SECOND_STRICT_TRIPS[name], (name, pf.trips)
    # the two limits of the GPU test really differ on the large QPs and not on the small one
    assert G.SECOND_STRICT_TRIPS["strict3"] + 1 <= G.SECOND_SHORT_LIMIT < 71
    i = G.SECOND_NAMES.index("nothing_violated")
    assert (A[i] @ np.linalg.solve(H[i], -f[i]) < b[i] - 0.5).all()
    for i in (0, 5):  # the vertex QPs end on n rows: more than SECOND_SHORT_LIMIT ADDs
        assert bin(int(G.VERTEX_ORACLE_SETS[(n, m)][0 if i == 0 else 1], 16)).count("1") == n
    assert len({a.tobytes() for a in b}) == 6  # six distinct QPs


# ------------------------------------------------------------------- vertex
@functools.lru_cache(maxsize=None)
def _vertex_facts(n, m, B):
    H, f, A, b = G.vertex(n, m, B, G.vertex_seed(n), G.VERTEX_SCALE)
    return (H, f, A, b), [G.path_facts(H[i], f[i], A[i], b[i]) for i in range(B)], \
        [O.active_set_solve(H[i], f[i], A[i], b[i], max_iter=G.ORACLE_MAX_ITER) for i in range(B)]


@pytest.mark.parametrize("n,m,B", G.VERTEX)
def test_vertex_paths_cross_the_seams(n, m, B):
    (H, f, A, b), facts, refs = _vertex_facts(n, m, B)
    for i, (pf, ref) in enumerate(zip(facts, refs)):
        assert ref.status == 0, i
        kkt = max(float(v.max()) for v in O.kkt_residuals(H[i:i + 1], f[i:i + 1], A[i:i + 1], b[i:i + 1], ref.x[None],
                                                          ref.lam[None]).values())
        lam_min, slack_min = ref.lam[ref.active].min(), (b[i] - A[i] @ ref.x)[~ref.active].min()
        print(f"vertex ({n},{m}) QP {i}: {int(ref.active.sum())} active rows, oracle KKT {kkt:.1e}, smallest active "
              f"multiplier {lam_min:.3g}, smallest inactive slack {slack_min:.3g}; model trips {pf.trips} DROPs "
              f"{pf.drops} " + " ".join(f"{c[6:]} {getattr(pf, c)}" for c in G.DROP_COUNTERS))
        assert kkt <= 1e-9
        assert pf.final == tuple(np.nonzero(ref.active)[0]), i
        assert lam_min > MARGIN and slack_min > MARGIN, i
        assert pf.trips + 1 <= G.iteration_cap(n, m)
    total = tuple(sum(getattr(pf, c) for pf in facts) for c in G.DROP_COUNTERS)
    print(f"vertex ({n},{m}): over the batch " + " ".join(f"{c[6:]} {v}" for c, v in zip(G.DROP_COUNTERS, total)))
    assert all(v > 0 for v in total), total
    full = sum(int(ref.active.sum()) == n for ref in refs)
    if (n, m) == (80, 200):
        assert full == B
    key = (n, m)
    assert tuple(G.mask_hex(ref.active) for ref in refs) == G.VERTEX_ORACLE_SETS[key]
    assert tuple(pf.trips for pf in facts) == G.VERTEX_MODEL_TRIPS[key]
    assert tuple(pf.drops for pf in facts) == G.VERTEX_MODEL_DROPS[key]
    assert total == G.VERTEX_DROP_COUNTERS[key]
    assert full == G.VERTEX_FULL_SETS[key]
    assert sum(pf.drops > 0 for pf in facts) == G.VERTEX_QPS_WITH_A_DROP[key]


# ---------------------------------------------------------------------- box
@pytest.mark.parametrize("n", G.BOX_N)
def test_box_sets_past_ql(n):
    H, f, lb, ub = G.box_full(n, G.BOX_B, G.box_seed(n))
    A, b = G.box_rows(lb, ub)
    H0 = G.box_shared_family(n)[0]
    assert np.array_equal(H0, H[0])
    for what, Hs, nact_c, over_c in (("box_full", H, G.BOX_ORACLE_NACT, G.BOX_OVER_QL),
                                     ("on QP 0's H", [H0] * G.BOX_B, G.BOX_SHARED_ORACLE_NACT, G.BOX_SHARED_OVER_QL)):
        refs = [O.active_set_solve(Hs[i], f[i], A[i], b[i], max_iter=G.ORACLE_MAX_ITER) for i in range(G.BOX_B)]
        assert all(r.status == 0 for r in refs)
        nact = tuple(int(r.active.sum()) for r in refs)
        over = sum(k > G.QL for k in nact)
        print(f"box n={n} {what}: active bounds {nact}, {over} QPs with more than QL = {G.QL}")
        assert nact == nact_c[n] and over == over_c[n]
        assert over >= 4
