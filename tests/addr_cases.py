"""TEST INFRASTRUCTURE ONLY: the inputs of tests/test_gpu_dense_addressing.py,
shared with tools/record_addr_golden.py (numpy, no GPU).

Every case is a batch of QPs with a planted, exact solution (tests/planted.py),
chosen to be the smallest at which the n <= 16 kernel's addressing -- a scalar
base per group of four QPs plus a 32-bit offset per lane -- or its scalar
bounds over the four active-set sizes of a wave can go wrong:

  b1 b2 b3 b5 b67  batches of 1, 2, 3, 5 and 67 at (16, 32): a ragged last
                   group, one group, several groups
  offset           9 = 4 * 2 + 1 QPs at (16, 32), every array a view that
                   starts 3 QPs into a larger allocation
  16x16 16x20 12x32 5x7 16x0 5x0
                   the other five instantiations and the padded forms' clamps;
                   m = 0 has no A or b at all
  eq               qpb_solve_eq at (16, 32, meq = 3)
  active           waves whose QPs end with 0, 1, 8, 9 and 16 active rows,
                   mixed: both groups of the x gather, its 8-row boundary, a
                   QP with q = 0 next to one with q = 16
"""
from typing import NamedTuple, Optional

import numpy as np

import planted

OFFSET_SKIP = 3  # QPs before the `offset` case's first one in its allocation
# active rows of the QPs of the `active` case, four per wave
ACTIVE_WAVES = [(0, 16, 8, 9), (1, 0, 16, 9), (8, 1, 0, 16), (0, 1, 0, 1), (0, 0, 0, 0), (8, 8, 1, 0), (9, 0, 0, 0)]


class Case(NamedTuple):
    H: np.ndarray
    f: np.ndarray
    A: Optional[np.ndarray]  # None: m = 0
    b: Optional[np.ndarray]
    x: np.ndarray            # the planted solution
    meq: int = 0


def box_with_active(seed: int, k: int, n: int = 16) -> Case:
    """One QP over lb <= x <= ub as 2 n rows [I; -I]: k variables sit on a bound
    with a multiplier in [1, 4] of that bound's sign, the others strictly
    inside, so the active set at the solution is exactly those k rows."""
    rs = np.random.default_rng([seed, n, k, 77])
    H = planted._spd(rs, n)
    x = rs.integers(-3, 4, n).astype(np.float64)
    lb = x - rs.integers(1, 6, n)
    ub = x + rs.integers(1, 6, n)
    on = rs.permutation(n)[:k]
    side = rs.choice([-1.0, 1.0], n)
    mu = np.zeros(n)
    mu[on] = planted._mult(rs, k) * side[on]
    ub[on] = np.where(side[on] > 0, x[on], ub[on])
    lb[on] = np.where(side[on] < 0, x[on], lb[on])
    A = np.concatenate([np.eye(n), -np.eye(n)])
    return Case(H, -H @ x - mu, A, np.concatenate([ub, -lb]), x)


def _dense(n, m, count):
    p, _ = planted.dense_batch(n, m, count)
    return Case(p.H, p.f, p.A, p.b, p.x)


def _unconstrained(n, count):
    p, _ = planted.dense_batch(n, 2 * n, count)
    return Case(p.H, -np.einsum("bij,bj->bi", p.H, p.x), None, None, p.x)


def cases():
    """name -> Case, in the order the golden file holds them."""
    out = {}
    big = _dense(16, 32, 67)
    for B in (1, 2, 3, 5, 67):
        out[f"b{B}"] = Case(*(a[:B] for a in big[:5]))
    out["offset"] = Case(*(a[OFFSET_SKIP:OFFSET_SKIP + 9] for a in big[:5]))
    for n, m in ((16, 16), (16, 20), (12, 32), (5, 7)):
        out[f"{n}x{m}"] = _dense(n, m, 13)
    out["16x0"] = _unconstrained(16, 13)
    out["5x0"] = _unconstrained(5, 13)
    e, _ = planted.eq_batch(16, 32, 3, 13)
    out["eq"] = Case(e.H, e.f, e.A, e.b, e.x, 3)
    qs = [box_with_active(1000 + i, k) for i, k in enumerate(k for w in ACTIVE_WAVES for k in w)]
    out["active"] = Case(*(np.stack([q[j] for q in qs]) for j in range(5)))
    return out


def input_digest(cs) -> str:
    """sha256 over every case's inputs: the goldens belong to exactly these bits."""
    import hashlib
    h = hashlib.sha256()
    for name, c in cs.items():
        h.update(name.encode())
        for a in (c.H, c.f, c.A, c.b):
            if a is not None:
                h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


def solve_case(qpb, c: Case, offset: bool = False):
    """qpb_solve (qpb_solve_eq for meq > 0) of one case on the device -> the five
    outputs as numpy arrays.  offset: inputs and outputs are views that start
    OFFSET_SKIP QPs into larger allocations (filled with NaN around them)."""
    import torch
    dev = torch.device("cuda", 0)

    def put(a, fill=float("nan")):
        if a is None:
            return None
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        if not offset:
            return t
        big = torch.full((OFFSET_SKIP + t.shape[0] + 2,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=dev)
        big[OFFSET_SKIP:OFFSET_SKIP + t.shape[0]] = t
        return big[OFFSET_SKIP:OFFSET_SKIP + t.shape[0]]

    H, f, A, b = (put(a) for a in (c.H, c.f, c.A, c.b))
    out = whole = None
    if offset:
        B, n = c.f.shape
        whole = qpb._empty_solution(OFFSET_SKIP + B + 2, n, c.b.shape[1], dev)
        for t in whole:
            t.zero_()
        out = type(whole)(*(t[OFFSET_SKIP:OFFSET_SKIP + B] for t in whole))
    if c.meq:
        sol = qpb.solve_eq(H, f, A, b, c.meq, out=out)
    elif A is None:
        sol = qpb.solve(H, f, out=out)
    else:
        sol = qpb.solve(H, f, A, b, out=out)
    torch.cuda.synchronize()
    if whole is not None:  # nothing was stored outside the views
        for t in whole:
            assert not t[:OFFSET_SKIP].any() and not t[OFFSET_SKIP + len(c.f):].any()
    return {k: np.ascontiguousarray(getattr(sol, k).cpu().numpy()) for k in ("x", "lam", "active", "status", "iters")}
