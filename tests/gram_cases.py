"""TEST INFRASTRUCTURE ONLY: inputs that take the n <= 128 Gram kernel
(csrc/qpb_gi_gram.hip) to active sets past 64 and 70 rows, and the facts about
each input's path that make it worth running (numpy, no GPU).

The kernel runs code above two sizes of the active set q that it does not run
below them:

  q > WAVE = 64   a DROP's lane l carries rows l and l + 64 of Z (wave 0) and
                  of lamb / iamb (wave 3): the second arm is dead below 65
  q > QL = 70     Q1's rows 70 .. 127 live in a per-workgroup global scratch,
                  not in LDS: the d pass's block of positions 68 .. 71, the w
                  pass's tail loop, the ADD's store and the DROP's chain across
                  the 69 | 70 seam

Families:

  strict_dense   a planted QP (tests/planted.py's pieces) with k independent
                 tight rows, all with lam* > 0, slack >= 1 elsewhere: the
                 active set is unique and the solve passes through every q < k
  vertex         H = I + 0.1 B^T B / n, f ~ scale N(0, I): at scale = 1000 the
                 solve ends on n active rows after tens of DROPs at every size
  box_full       lb <= x <= ub where most variables end on a bound

path_facts runs tools/gi_select_sim.py's numpy model of the kernel's method
with its trace and counts where the DROPs fell.  tests/test_gram_cases.py
asserts, on the CPU, that the constants at the end of this module are what the
model and the oracle give today; tests/test_gpu_gram_large_sets.py reads them,
so that no GPU test runs the model and no threshold comes from the kernel.
"""
from __future__ import annotations

import os
import sys
from typing import NamedTuple

import numpy as np

import planted as P

_TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if _TOOLS not in sys.path:
    sys.path.insert(0, _TOOLS)

# The two seams, derived in one place from qpb_gi_gram.hip's constants
# (tests/test_gram_cases.py parses them out of the file and compares):
# NT = 512 threads are 8 wavefronts of NT / 8 = 64 lanes, so a lane of a DROP
# carries positions l and l + 64; QL = (OFF_BUF - OFF_ROWS) / QS = (LDS_D - NBUF
# - LP) / QS is the number of Q1 rows that fit in LDS.
NT, NB, LDS_D, NBUF, QS = 512, 128, 20480, 2136, 144
LP = NB * (NB + 1) // 2
WAVE = NT // 8
QL = (LDS_D - NBUF - LP) // QS


def iteration_cap(n: int, m: int) -> int:
    """The library's default max_iter (qpb.h)."""
    return 4 * (n + m) + 8


# ------------------------------------------------------------------ families
def strict_dense(n: int, m: int, k: int, seed: int) -> P.Planted:
    """One planted QP with k <= n independent tight rows, each with an integer
    lam* in [1, 4], and an integer slack in [1, 5] on every other row; the rows
    are permuted.  Integer data: b, f and the KKT residuals of (x*, lam*) are
    exact.  Strictly complementary and independent: the active set is unique."""
    rs = np.random.default_rng([seed, n, m, k, 6])
    H = P._spd(rs, n)
    x = rs.integers(-3, 4, n).astype(np.float64)
    A = P._rows(rs, m, n)
    A[:k] = P._independent_rows(rs, k, n)
    lam = np.zeros(m)
    lam[:k] = P._mult(rs, k)
    tight = np.arange(m) < k
    b = A @ x + np.where(tight, 0.0, rs.integers(1, 6, m))
    f = -H @ x - A.T @ lam
    p = rs.permutation(m)
    return P.Planted(H, f, A[p], b[p], x, lam[p], tight[p], -np.ones(m, np.int64))


def strict_batch(n: int, m: int, k: int, seeds) -> P.Planted:
    qs = [strict_dense(n, m, k, s) for s in seeds]
    return P.Planted(*(np.stack(v) for v in zip(*qs)))


def vertex(n, m, B, seed, scale=100.0):
    """H = I + 0.1 BᵀB/n, f ~ scale·N(0, I), m unit-norm random rows with
    b ~ U[0.1, 1): the unconstrained minimiser lies far outside, so the solve
    adds constraints up to a full active set (q = n, a vertex) and drops some
    on the way -- including DROPs taken with q = n -- the paths where the
    kernels' exchange row shares R's column 0 and the Givens parameters stay
    in registers."""
    rs = np.random.default_rng(seed)
    Bm = rs.standard_normal((B, n, n))
    H = np.eye(n) + 0.1 * np.einsum("bki,bkj->bij", Bm, Bm) / n
    f = scale * rs.standard_normal((B, n))
    A = rs.standard_normal((B, m, n))
    A /= np.linalg.norm(A, axis=2, keepdims=True)
    b = rs.uniform(0.1, 1.0, (B, m))
    return H, f, A, b


def box_full(n, B, seed):
    """(H, f, lb, ub) of B box QPs on the unit box in two halves:
    first half: H = I + BᵀB/n, f ~ 1.25 n N(0, I) -> most variables at a bound;
    second half: H = 0.01 I + BᵀB/n, f ~ N(0, I) -> strongly coupled, the
    dual path drops bounds it added (the numpy G-I model: 39-100 of 128)"""
    rs = np.random.default_rng(seed)
    Bm = rs.standard_normal((B, n, n))
    h = B // 2
    H = np.einsum("bki,bkj->bij", Bm, Bm) / n
    H[:h] += np.eye(n)
    H[h:] += 0.01 * np.eye(n)
    f = rs.standard_normal((B, n))
    f[:h] *= 1.25 * n
    lb, ub = -np.ones((B, n)), np.ones((B, n))
    return H, f, lb, ub


def box_rows(lb, ub):
    """The box as A x <= b with A = [I; -I], b = [ub; -lb] (qpb.h's row order)."""
    B, n = lb.shape
    I = np.broadcast_to(np.eye(n), (B, n, n))
    return np.concatenate([I, -I], axis=1), np.concatenate([ub, -lb], axis=1)


# ---------------------------------------------------------------- path facts
class PathFacts(NamedTuple):
    final: tuple          # the model's final active set, sorted rows; None if the model failed
    trips: int            # ADDs + DROPs (the kernel's iters is one more on the fp64 routes)
    max_q: int            # the largest size the set reached
    drops: int
    drops_wave_arm: int   # DROPs with k < WAVE <= q - 1: the shift crosses into the l + 64 arm
    drops_seam: int       # DROPs with k < QL <= q - 1: the Q1 chain walks across the 69 | 70 seam
    drops_past_wave: int  # DROPs with k >= WAVE: the second arm alone
    drops_past_ql: int    # DROPs with k >= QL: the chain in the scratch alone
    drops_at_n: int       # DROPs taken at q == n
    add_q: frozenset      # the sizes q at which an ADD happened


def path_facts(H, f, A, b) -> PathFacts:
    """One QP through tools/gi_select_sim.py::gi (rule `anorm`, the kernel's)
    with the library's default iteration cap, and where its steps fell."""
    from gi_select_sim import gi
    n, m = len(f), len(b)
    trace = []
    it, adds, drops, W = gi(H, f, A, b, "anorm", trace=trace, max_it=iteration_cap(n, m))
    dr = [(q, k) for q, what, k in trace if what == "drop"]
    assert len(dr) == drops and it == adds + drops
    return PathFacts(
        final=None if W is None else tuple(int(i) for i in W), trips=int(it),
        max_q=max([q + (what == "add") for q, what, _ in trace], default=0), drops=len(dr),
        drops_wave_arm=sum(k < WAVE <= q - 1 for q, k in dr), drops_seam=sum(k < QL <= q - 1 for q, k in dr),
        drops_past_wave=sum(k >= WAVE for q, k in dr), drops_past_ql=sum(k >= QL for q, k in dr),
        drops_at_n=sum(q == n for q, k in dr), add_q=frozenset(q for q, what, _ in trace if what == "add"))


DROP_COUNTERS = ("drops_wave_arm", "drops_seam", "drops_past_wave", "drops_past_ql", "drops_at_n")


def mask_hex(mask) -> str:
    """A bool row mask as the hex of sum 2^i over its set rows."""
    return format(sum(1 << int(i) for i in np.nonzero(mask)[0]), "x")


def hex_mask(h: str, m: int) -> np.ndarray:
    v = int(h, 16)
    return np.array([(v >> i) & 1 for i in range(m)], dtype=bool)


# ------------------------------------------------------------------ the cases
# test_strict_sets: (n, m, k), two seeds per shape in one launch
STRICT = [(65, 66, 65), (71, 80, 71), (72, 144, 72), (100, 120, 100),
          (127, 255, 127), (128, 256, 70), (128, 256, 71), (128, 256, 128)]
STRICT_SEEDS = (1, 2)
# test_vertex_drops_past_the_seams: (n, m, B); seed 500 + n, scale 1000
VERTEX = [(80, 200, 6), (128, 256, 6)]
VERTEX_SCALE = 1000.0
# test_box_large_sets: n; B = 8, seed 900 + n
BOX_N = (72, 100, 128)
BOX_B = 8
ORACLE_MAX_ITER = 2000  # one (128, 256) vertex QP needs 510 primal iterations, above the oracle's default 500


def vertex_seed(n: int) -> int:
    return 500 + n


def box_seed(n: int) -> int:
    return 900 + n


def box_shared_family(n: int):
    """box_full's batch on ONE H, QP 0's (the stride-0 form of
    qpb_solve_box_shared): (H0 (n, n), f, lb, ub)."""
    H, f, lb, ub = box_full(n, BOX_B, box_seed(n))
    return np.ascontiguousarray(H[0]), f, lb, ub


# test_second_qp_of_a_workgroup: six distinct QPs of one shape that leave the workgroup's LDS and scratch in
# different states (a full set reached through DROPs, a set one row into the scratch, a tiny set, none at
# all, the loop's early INFEASIBLE break, a full set again)
SECOND_SHAPE = (80, 200)
SECOND_NAMES = ("vertex", "strict71", "strict3", "nothing_violated", "farkas", "vertex_again")
SECOND_SHORT_LIMIT = 40  # a max_iter at which the large QPs stop in mid-flight
SECOND_STRICT_TRIPS = {"strict71": 73, "strict3": 3}  # the model's trips on strict_dense(80, 200, k, 1)


def second_qp_cases():
    """(H, f, A, b) of SECOND_NAMES' six QPs, stacked, and the two planted QPs.
    nothing_violated is vertex QP 2 with b = A xu + 1 at the unconstrained
    minimiser xu; farkas is oracle.family_farkas's b_inf (k = 5)."""
    import oracle as O
    n, m = SECOND_SHAPE
    Hv, fv, Av, bv = vertex(n, m, 6, vertex_seed(n), VERTEX_SCALE)
    s71, s3 = strict_dense(n, m, 71, 1), strict_dense(n, m, 3, 1)
    b0 = Av[2] @ np.linalg.solve(Hv[2], -fv[2]) + 1.0
    Hf, ff, Af, b_inf = O.family_farkas(1200 + n + m, 1, n, m, 5)[:4]
    qps = [(Hv[0], fv[0], Av[0], bv[0]), s71[:4], s3[:4], (Hv[2], fv[2], Av[2], b0),
           (Hf[0], ff[0], Af[0], b_inf[0]), (Hv[1], fv[1], Av[1], bv[1])]
    return tuple(np.stack(v) for v in zip(*qps)), {"strict71": s71, "strict3": s3}


# ------------------------------------------------ what the model and the oracle give
# Recomputed and compared by tests/test_gram_cases.py (CPU); read by the GPU tests.

# strict_dense(n, m, k, seed) for seed in STRICT_SEEDS: the model's trips (ADDs + DROPs); its final set is the
# planted one and its largest q is k on every entry
STRICT_MODEL_TRIPS = {(65, 66, 65): (69, 71), (71, 80, 71): (79, 75), (72, 144, 72): (80, 80), (100, 120, 100): (110, 120),
                      (127, 255, 127): (141, 145), (128, 256, 70): (70, 70), (128, 256, 71): (75, 73),
                      (128, 256, 128): (146, 136)}

# vertex(n, m, B, 500 + n, 1000.0): per QP the oracle's active set (mask_hex), the model's trips and DROPs,
# and over the batch the five DROP counters, the QPs that end with n active rows and the QPs with a DROP
VERTEX_ORACLE_SETS = {
    (80, 200): ('b81461e1a5082820a7fb108b32001c3da3966b8a5207540ec8',
                '2b0c5204c6c70299857168ce0644521604f3942118192ad2fd',
                'aa3dc3404c0d4289114bc7082cb6d666ce0180f6210382e125',
                'cd130a0813447040798a55f90912e673332d4e12d0674b84',
                '10ee998021d85ab04b5b92ae191b4040da503085618a345ec4',
                '60b548091c14a8ab1b765c8d50821e189222cd2526493e0b24'),
    (128, 256): ('cb969d54c004b3b7e1993bdb680f426b850de72147bfc582c81110cc58c82499',
                 'e089a1c467b0a550f61fd7e0387f610962a2d5146d1a087afd8abe25fceffd2',
                 '468b1869393f400a1682fd17e0a4bba1ec6ed2593aae9fa6e7cef091e18c5dac',
                 'e43a1edd082efa4ac648b4c001b5b56c04e79c76552bb7243c94e8299bf7daa5',
                 'f1a48195295f37a957a5c82ee48ead58bd6059a68154e4fa82a0cb58ed2ed8dd',
                 '6212e6a0881899fce32f63a6dbdcf308da4909ac6b7b880d8e64a035b27038de')}
VERTEX_MODEL_TRIPS = {(80, 200): (210, 196, 174, 184, 200, 184), (128, 256): (185, 232, 278, 188, 233, 175)}
VERTEX_MODEL_DROPS = {(80, 200): (65, 58, 47, 52, 60, 52), (128, 256): (34, 52, 75, 31, 53, 27)}
VERTEX_DROP_COUNTERS = {(80, 200): (135, 177, 154, 107, 93), (128, 256): (137, 144, 127, 116, 7)}  # in DROP_COUNTERS' order
VERTEX_FULL_SETS = {(80, 200): 6, (128, 256): 2}
VERTEX_QPS_WITH_A_DROP = {(80, 200): 6, (128, 256): 6}

# box_full(n, 8, 900 + n) on A = [I; -I]: per QP the number of active bounds in the oracle's set, and the
# number of QPs with more than QL of them
BOX_ORACLE_NACT = {72: (72, 71, 71, 72, 41, 43, 43, 42), 100: (100, 97, 99, 100, 59, 60, 58, 58),
                   128: (127, 126, 125, 126, 75, 71, 76, 82)}
BOX_OVER_QL = {72: 4, 100: 4, 128: 8}
# box_shared_family(n) (every QP on QP 0's H): the same two
BOX_SHARED_ORACLE_NACT = {72: (72, 71, 71, 72, 8, 9, 11, 4), 100: (100, 97, 97, 100, 15, 7, 11, 13),
                          128: (127, 126, 127, 125, 21, 15, 17, 13)}
BOX_SHARED_OVER_QL = {72: 4, 100: 4, 128: 4}
