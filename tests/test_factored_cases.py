"""The inputs of tests/test_gpu_factored.py meet the condition its active-set
comparison rests on (no GPU): on every shape and batch of factored_cases, the
oracle solves every QP and at least 95 % of them are strictly complementary --
the smallest multiplier on an active inequality and the smallest slack on an
inactive row both exceed 1e-8 of their scale -- so two correct solvers must
report the same active set on them."""
import numpy as np
import pytest

import eq_oracle as EO
import factored_cases as FC
import shared_cases as SC


@pytest.mark.parametrize("n,m,meq", FC.SHAPES)
def test_family_is_strictly_complementary(n, m, meq):
    for B in FC.BATCHES:
        H0, f, A0, b = SC.family(B, n, m, meq)
        x, lam, act, strict = FC.oracle(B, n, m, meq)
        share = strict.mean()
        print(f"({n},{m},{meq}) B={B}: strictly complementary {int(strict.sum())}/{B}, "
              f"active rows {act.sum(axis=1).min() if m else 0}..{act.sum(axis=1).max() if m else 0}")
        assert share >= FC.MIN_STRICT_SHARE, (B, share)
        if m:
            # the oracle's own answer is a KKT point of the shared problem at the test's bar
            res = EO.kkt_mixed(SC.expand(H0, B), f, SC.expand(A0, B), b, meq, x, lam)
            assert all(v.max() <= FC.KKT_TOL for v in res.values()), {k: v.max() for k, v in res.items()}
            assert act[:, :meq].all()
    if m > meq:
        assert any(FC.oracle(B, n, m, meq)[2][:, meq:].any() for B in FC.BATCHES), "no inequality is ever active"
