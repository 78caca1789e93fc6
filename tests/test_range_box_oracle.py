"""The qpb_solve_range_box test family (tests/range_box_oracle.py), on the CPU:
what the GPU tests rely on when they compare masks bit for bit.  At every
shape, 24 QPs: each is solved (status 0, none left out), the active set is
unambiguous (active |lam| >= 1, inactive slack >= 1e-3), and both sides of the
variables' bounds and of the general rows are active somewhere.
"""
import numpy as np
import pytest

import range_box_oracle as BO

COUNT = 24


@pytest.mark.parametrize("n,mg,meq", BO.SHAPES)
def test_family(n, mg, meq):
    (H, f, G, bl, bu, lb, ub, xc), (A, lo, hi), refs = BO.box_reference(COUNT, n, mg, meq)
    m = mg + n
    assert len(refs) == COUNT and A.shape == (COUNT, m, n)
    assert [r.status for r in refs] == [0] * COUNT
    assert (lb < xc).all() and (xc < ub).all()
    act = np.array([r.active for r in refs])
    low = np.array([r.lower for r in refs])
    lam = np.array([r.lam for r in refs])
    x = np.array([r.x for r in refs])
    ax = np.einsum("bij,bj->bi", A, x)
    slack = np.minimum(hi - ax, ax - lo)
    ineq = np.arange(m) >= meq
    min_lam = np.abs(lam[act]).min()
    min_slack = slack[~act & ineq].min() if (~act & ineq).any() else np.inf
    print(f"({n},{mg},{meq}): active rows up {int((act & ~low)[:, meq:mg].sum())} lo {int(low[:, :mg].sum())}, "
          f"bounds up {int((act & ~low)[:, mg:].sum())} lo {int(low[:, mg:].sum())}, "
          f"min active |lam| {min_lam:.3g}, min inactive slack {min_slack:.3g}")
    assert min_lam >= 1.0
    assert min_slack >= 1e-3
    assert not (low & ~act).any() and not low[:, :meq].any()
    assert (lam[~act] == 0).all()
    # a variable's bound on each side
    assert (act & ~low)[:, mg:].any() and low[:, mg:].any()
    # ... and a general row on each side where there is one that is no equality
    if mg > meq:
        assert (act & ~low)[:, meq:mg].any() and low[:, meq:mg].any()
