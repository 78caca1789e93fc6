"""The qpb_solve_range oracle (tests/range_oracle.py) on the CPU: the pair
mapping on one-variable QPs whose answers are known by hand, and the facts about
the test family that the GPU tests rely on -- every QP solvable, both sides
active about equally often, and many rows active on the side opposite to the
one violated at the unconstrained minimum (the rows that reach a kernel's
re-orientation).  Re-asserted here so that nobody can move the family to where
a side goes untested."""
import numpy as np
import pytest

import range_oracle as RO

B = 67
SHAPES = [(16, 32, 0), (16, 32, 4), (16, 16, 3), (7, 13, 3), (20, 33, 5), (32, 64, 8)]


def one_var(f, bl, bu):
    """min 1/2 x^2 + f x  s.t.  bl <= x <= bu, from xc = (bl + bu) / 2"""
    return RO.range_solve([[1.0]], [f], [[1.0]], [bl], [bu], 0, [(bl + bu) / 2.0])


def test_clamp_from_above():
    r = one_var(-5.0, -1.0, 2.0)  # the free minimum is x = 5
    assert r.status == 0 and np.allclose(r.x, [2.0])
    assert np.allclose(r.lam, [3.0])  # x + f + lam = 0
    assert r.active.tolist() == [True] and r.lower.tolist() == [False]


def test_clamp_from_below():
    r = one_var(4.0, -1.0, 2.0)  # the free minimum is x = -4
    assert r.status == 0 and np.allclose(r.x, [-1.0])
    assert np.allclose(r.lam, [-3.0])
    assert r.active.tolist() == [True] and r.lower.tolist() == [True]


def test_interior():
    r = one_var(-0.5, -1.0, 2.0)
    assert r.status == 0 and np.allclose(r.x, [0.5])
    assert np.allclose(r.lam, [0.0])
    assert r.active.tolist() == [False] and r.lower.tolist() == [False]


def test_pairs_and_back():
    A = np.arange(6.0).reshape(3, 2)
    A2, b2 = RO.to_pairs(A, [9.0, -1.0, np.nan], [1.0, np.inf, 3.0], 1)
    assert np.array_equal(A2, np.vstack([A[:1], A[1:], -A[1:]]))
    assert np.array_equal(b2, [1.0, np.inf, 3.0, 1.0, np.inf])
    lam, act, low = RO.from_pairs([-2.0, 0.0, 4.0, 5.0, 0.0], [1, 0, 1, 1, 0], 3, 1)
    assert lam.tolist() == [-2.0, -5.0, 4.0]
    assert act.tolist() == [True, True, True] and low.tolist() == [False, True, False]


def test_bits_round_trip():
    rng = np.random.default_rng(3)
    for m in (1, 13, 32, 33, 64):
        mask = rng.random((5, m)) < 0.4
        words = RO.pack_bits(mask)
        assert words.shape == (5, (m + 31) // 32) and words.dtype == np.uint32
        assert np.array_equal(RO.unpack_bits(words, m), mask)
        assert np.array_equal(RO.unpack_bits(words.view(np.int32), m), mask)


def test_certificate_sees_a_wrong_side():
    r = one_var(4.0, -1.0, 2.0)
    H, f, A = np.ones((1, 1, 1)), np.array([[4.0]]), np.ones((1, 1, 1))
    bl, bu = np.array([[-1.0]]), np.array([[2.0]])
    good = RO.kkt_range(H, f, A, bl, bu, 0, r.x[None], r.lam[None])
    assert max(v.max() for v in good.values()) <= 1e-12
    bad = RO.kkt_range(H, f, A, bl, bu, 0, r.x[None], -r.lam[None])  # the multiplier of the other side
    assert bad["dual"].max() > 0.1 and bad["stat"].max() > 0.1
    out = RO.kkt_range(H, f, A, bl, bu, 0, np.array([[-1.5]]), np.array([[-2.5]]))  # below bl
    assert out["prim"].max() > 0.1


@pytest.mark.parametrize("n,m,meq", SHAPES)
def test_family_facts(n, m, meq):
    H, f, A, bl, bu, xc, refs = RO.range_reference(B, n, m, meq)  # asserts every QP OK
    ax = np.einsum("bij,bj->bi", A, xc)
    assert (bu[:, meq:] - ax[:, meq:]).min() >= 1.0 and (ax[:, meq:] - bl[:, meq:]).min() >= 1.0
    assert np.array_equal(bl[:, :meq], bu[:, :meq])
    x = np.stack([r.x for r in refs])
    lam = np.stack([r.lam for r in refs])
    cert = RO.kkt_range(H, f, A, bl, bu, meq, x, lam)
    assert max(v.max() for v in cert.values()) <= 1e-9, {k: v.max() for k, v in cert.items()}
    up, lo, opp = RO.side_counts(B, n, m, meq)
    print(f"n={n} m={m} meq={meq}: {up} upper, {lo} lower, {opp} opposite to x0's side")
    assert up > 0 and lo > 0 and 0.6 <= up / lo <= 1.6, (up, lo)
    assert 57 <= opp <= 476, opp
    if (n, m, meq) == (16, 32, 0):
        assert (up, lo) == (407, 380)
    for r in refs:  # lower is a subset of active, never an equality; lam's sign names the side
        assert not (r.lower & ~r.active).any() and not r.lower[:meq].any()
        nz = r.lam[meq:] != 0
        assert np.array_equal((r.lam[meq:] < 0)[nz], r.lower[meq:][nz])
