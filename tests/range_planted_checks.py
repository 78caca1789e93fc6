"""TEST INFRASTRUCTURE ONLY: what a qpb_solve_range answer must satisfy on a
planted range batch (tests/planted.py's PlantedRange; numpy, no GPU).

At a degenerate vertex the active set is not unique, so `check` asserts what is:

  status OK on every QP, 1 <= iters <= 4 (n + m) + 8 (no QP is excused)
  x within 1e-9 relative of the planted x* (integer data, cond(H) < 12)
  range_oracle.kkt_range of the answer's own (x, lam) <= 1e-9, all four residuals
  lower within active, lower clear on rows < meq, every equality active,
    lam == 0.0 outside active
  active within the tight rows, per side and at lam = 0 too: an active row of
    positive width has `lower` set only if it is tight at bl (side -1) and
    clear only if it is tight at bu (side +1); a zero-width row may carry either
  a nonzero lam on a row of positive width has the sign its side names
  A^T lam == A^T lam* within 1e-9 relative
  where rank(A[tight]) equals the number of tight rows (lam* is the only
    multiplier): every row with lam* != 0 is active, lam within 1e-9 of lam*
  at least one row of every `group` (dup triple, pinned pair, dup_bound pair) is active
  thin (not degenerate): active == (lam* != 0) and lower == (side == -1), bit for bit

tests/test_planted.py shows on the CPU that the planted answer passes and that
a flipped lower bit, a negated lam, a lam one slot off, an active bit on a slack
row and an x moved by 1e-6 do not.
"""
from __future__ import annotations

import numpy as np

import range_oracle as RO

X_TOL = 1e-9
KKT_TOL = 1e-9
OK = 0


def relx(x, xr):
    return np.abs(x - xr).max(axis=1) / np.maximum(1.0, np.abs(xr).max(axis=1))


def planted_answer(q, meq: int, iters: int = 2):
    """(x, lam, active, lower, status, iters) that a perfect solver could
    return: the planted pair, active where lam* != 0 (and on the equalities),
    lower where that row sits at bl (a zero-width row: where lam* < 0)."""
    B, m = q.lam.shape
    act = q.lam != 0
    act[:, :meq] = True
    low = act & ((q.side == -1) | ((q.side == 2) & (q.lam < 0)))
    low[:, :meq] = False
    return [q.x.copy(), q.lam.copy(), RO.pack_bits(act), RO.pack_bits(low), np.zeros(B, np.int32),
            np.full(B, iters, np.int32)]


def check(q, kinds, sol, what, meq: int = 0):
    """The module docstring's assertions on one launch.  q: a PlantedRange
    batch; sol: (x, lam, active words, lower words, status, iters) as numpy
    arrays.  Prints the worst figures, returns them with the masks."""
    x, lam, act, low, st, it = sol
    B, m, n = q.A.shape
    mask, lmask = RO.unpack_bits(act, m), RO.unpack_bits(low, m)
    tight = q.side != 0
    wide = q.side != 2
    ex = relx(x, q.x)
    worst = {k: float(v.max()) for k, v in RO.kkt_range(q.H, q.f, q.A, q.bl, q.bu, meq, x, lam).items()} \
        if (st == OK).all() else {}
    atl = np.einsum("bij,bi->bj", q.A, lam)
    atr = np.einsum("bij,bi->bj", q.A, q.lam)
    ea = relx(atl, atr)
    degenerate = int((tight.sum(axis=1) > mask.sum(axis=1)).sum())
    bits, nt = mask.sum(axis=1), tight.sum(axis=1)
    print(f"{what}: status {np.bincount(st, minlength=5).tolist()} x err {ex.max():.2e} "
          f"kkt {max(worst.values(), default=np.nan):.2e} A^T lam err {ea.max():.2e} iters {it.min()}..{it.max()} "
          f"degenerate {degenerate}/{B} QPs with a DROP {int((it > bits + 1).sum())} "
          f"set bits {bits.min()}..{bits.max()} lower bits {int(lmask.sum())} tight {nt.min()}..{nt.max()}")
    assert (st == OK).all(), (what, st, it)
    assert (it >= 1).all() and (it <= 4 * (n + m) + 8).all(), (what, it)
    assert ex.max() <= X_TOL, (what, ex)
    assert all(v <= KKT_TOL for v in worst.values()), (what, worst)
    assert not (lmask & ~mask).any(), what
    assert not lmask[:, :meq].any(), what
    assert mask[:, :meq].all(), what
    assert (lam[~mask] == 0.0).all(), (what, np.nonzero((lam != 0) & ~mask))
    assert not (mask & ~tight).any(), (what, np.nonzero(mask & ~tight))
    bad = mask & wide & np.where(lmask, q.side != -1, q.side != 1)
    assert not bad.any(), (what, "active on a side that is not tight", np.nonzero(bad))
    nz = (lam != 0) & wide
    assert (np.sign(lam[nz]) == q.side[nz]).all(), (what, np.nonzero(nz & (np.sign(lam) != q.side)))
    assert ea.max() <= X_TOL, (what, ea)
    for i, kind in enumerate(kinds):
        for g in range(int(q.group[i].max()) + 1):
            assert mask[i, q.group[i] == g].any(), (what, i, kind, "no row of group", g)
        if np.linalg.matrix_rank(q.A[i][tight[i]]) == tight[i].sum():
            need = q.lam[i] != 0
            assert mask[i, need].all(), (what, i, kind, np.nonzero(need & ~mask[i]))
            assert np.abs(lam[i] - q.lam[i]).max() <= X_TOL * (1.0 + np.abs(q.lam[i]).max()), (what, i, kind)
        if kind == "thin":
            assert np.array_equal(mask[i], q.lam[i] != 0), (what, i, "thin: active")
            assert np.array_equal(lmask[i], q.side[i] == -1), (what, i, "thin: lower")
    return {"x": float(ex.max()), "kkt": max(worst.values()), "atl": float(ea.max()), "degenerate": degenerate,
            "active": mask, "lower": lmask}
