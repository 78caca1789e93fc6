"""The conditions the tests of qpb_solve_range_factored put on their own inputs
(tests/range_factored_cases.py), checked on the CPU at every shape and batch:
the oracle solves every QP, nearly every QP is strictly complementary (so that
`active` and `lower` can be compared bit for bit), and both sides of the
two-sided rows are exercised."""
import numpy as np
import pytest

import range_factored_cases as RF


@pytest.mark.parametrize("n,m,meq", RF.SHAPES)
def test_family_conditions(n, m, meq):
    for B in RF.BATCHES:
        H0, f, A0, bl, bu, xc = RF.family(B, n, m, meq)
        x, lam, act, low, strict, status = RF.oracle(B, n, m, meq)
        assert (status == 0).all(), (B, status)
        assert strict.mean() >= RF.MIN_STRICT_SHARE, (B, strict.mean())
        if m == 0:
            continue
        # the family's own point is strictly inside on both sides, the equalities hold at it
        ax = xc @ A0.T
        assert (bu[:, meq:] - ax[:, meq:] >= 1.0 - 1e-9).all() and (ax[:, meq:] - bl[:, meq:] >= 1.0 - 1e-9).all()
        assert np.array_equal(bl[:, :meq], bu[:, :meq]) and np.abs(ax[:, :meq] - bu[:, :meq]).max(initial=0.0) <= 1e-9
        assert not (low & ~act).any() and not low[:, :meq].any() and act[:, :meq].all()
        up_n, lo_n = int((act & ~low)[:, meq:].sum()), int(low[:, meq:].sum())
        print(f"({n},{m},{meq}) B={B}: strict {int(strict.sum())}/{B}, active rows >= meq: {up_n} upper / {lo_n} lower")
        if B == 67:
            assert min(up_n, lo_n) >= RF.MIN_SIDE_SHARE * (up_n + lo_n) and up_n + lo_n > 0, (up_n, lo_n)


def test_the_shapes_cover_every_load_path_and_both_classes():
    shapes = set(RF.SHAPES)
    assert RF.FULL_MR1 in shapes and RF.FULL_MR1[0] == 16 and RF.FULL_MR1[1] == 16  # n = 16, m = 16: FULL, MR = 1
    assert any(n == 16 and m == 32 for n, m, _ in shapes)                            # FULL, MR = 2
    assert any(n == 16 and 16 < m < 32 for n, m, _ in shapes)                        # n = 16, padded rows
    assert any(n < 16 and 0 < m <= 16 for n, m, _ in shapes)                         # padded n
    assert any(n > 16 for n, m, _ in shapes) and any(n <= 16 and m > 32 for n, m, _ in shapes)  # one QP per wavefront
    assert any(m == 0 for _, m, _ in shapes)
