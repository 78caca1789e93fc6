"""CPU checks of the batches behind tests/test_gpu_range_box_backward.py and
tests/test_gpu_range_box_dual_autograd.py, on the numpy oracle
(tests/range_box_oracle.py): the GPU tests compare bit patterns, which says
nothing unless the solves they differentiate have rows of G and variables
active on BOTH sides -- so that every one of gbl, gbu, glb and gub receives
routed elements -- and the finite differences need active sets that stay put.
"""
import numpy as np
import pytest

import range_box_bwd_cases as BC
import range_box_oracle as BO
import range_oracle as RO

COUNT = BC.COUNT  # the batch of the GPU tests' main cases, and of tests/test_range_box_oracle.py
FD_SHAPES = [(16, 16, 2), (12, 20, 0), (20, 9, 0)]  # the shapes differentiated numerically


def _sets(n, mg, meq):
    _, _, refs = BO.box_reference(COUNT, n, mg, meq)
    assert all(r.status == 0 for r in refs)
    act = np.array([r.active for r in refs])
    low = np.array([r.lower for r in refs])
    return act, low


@pytest.mark.parametrize("n,mg,meq", BO.SHAPES)
def test_both_sides_are_active_among_the_rows_and_the_variables(n, mg, meq):
    act, low = _sets(n, mg, meq)
    assert not (low & ~act).any()  # lower is a subset of active
    assert not low[:, :meq].any()  # never on an equality row
    rows_lo, rows_up = (act & low)[:, meq:mg].sum(), (act & ~low)[:, meq:mg].sum()
    vars_lo, vars_up = (act & low)[:, mg:].sum(), (act & ~low)[:, mg:].sum()
    print(f"({n},{mg},{meq}) B={COUNT}: rows at bl {rows_lo} at bu {rows_up}, variables at lb {vars_lo} at ub {vars_up}")
    assert vars_lo >= 1 and vars_up >= 1
    if mg > meq:  # the shape has inequality rows (not mg = 0, nor rows < meq only)
        assert rows_lo >= 1 and rows_up >= 1


@pytest.mark.parametrize("n,mg,meq", FD_SHAPES)
def test_margins_of_the_shapes_differentiated_numerically(n, mg, meq):
    """The margins of tests/test_gpu_range_box_autograd.py: at +-1e-6 the active
    sets do not move."""
    (H, f, G, bl, bu, lb, ub, xc), (A, lo, hi), refs = BO.box_reference(COUNT, n, mg, meq)
    act = np.array([r.active for r in refs])
    lam = np.array([r.lam for r in refs])
    ax = np.einsum("bij,bj->bi", A, np.array([r.x for r in refs]))
    slack = np.minimum(hi - ax, ax - lo)
    lam_min = np.abs(lam[act]).min()
    slack_min = slack[~act & (np.arange(mg + n) >= meq)].min()
    print(f"({n},{mg},{meq}) B={COUNT}: smallest active |lam| {lam_min:.3g}, smallest inactive slack {slack_min:.3g}")
    assert lam_min >= 1.0 and slack_min >= 1e-3


PREFIX = 48  # QPs of a larger batch handed to the oracle: what they show, the batch has


def _sides(count, n, mg, meq, share_h, share_g):
    H, f, G, bl, bu, lb, ub, xc, _ = BC.inputs(count, n, mg, meq, share_h, share_g)
    k = min(count, PREFIX)
    A, lo, hi = BO.materialise(G if G.ndim == 2 else G[:k], bl[:k], bu[:k], lb[:k], ub[:k], n)
    Hb = np.broadcast_to(H, (count, n, n))
    refs = [RO.range_solve(Hb[i], f[i], A[i], lo[i], hi[i], meq, xc[i]) for i in range(k)]
    assert all(r.status == 0 for r in refs)
    act = np.array([r.active for r in refs])
    low = np.array([r.lower for r in refs])
    return ((act & low)[:, meq:mg].sum(), (act & ~low)[:, meq:mg].sum(), (act & low)[:, mg:].sum(),
            (act & ~low)[:, mg:].sum())


@pytest.mark.parametrize("n,mg,meq", BC.SHARED_SHAPES)
@pytest.mark.parametrize("count", BC.SHARED_COUNTS)
@pytest.mark.parametrize("share_h,share_g", BC.SHARED_FORMS)
def test_the_shared_batches_have_both_sides_too(count, n, mg, meq, share_h, share_g):
    """The batches of the GPU tests' shared forms (one H, one G with bounds of its
    own, both; B = 24 and 261): among the first 48 QPs rows and variables are
    active on both sides, so all four bound arrays receive routed elements."""
    sides = _sides(count, n, mg, meq, share_h, share_g)
    print(f"({n},{mg},{meq}) B={count} H shared {share_h} G shared {share_g}: at bl, bu, lb, ub {sides}")
    assert min(sides) >= 1


@pytest.mark.parametrize("n,mg,meq", BC.RAGGED)
def test_the_ragged_batches(n, mg, meq):
    """B = 1, 3, 5 and 65 test the last wavefront of four QPs, not the routing: a
    batch of one QP cannot have every side active.  From B = 5 on these have."""
    for count in BC.RAGGED_COUNTS:
        sides = _sides(count, n, mg, meq, False, False)
        print(f"({n},{mg},{meq}) B={count}: at bl, bu, lb, ub {sides}")
        assert sum(sides) >= 1
        if count >= 5:
            assert min(sides) >= 1
