"""TEST INFRASTRUCTURE ONLY: the inputs and helpers the tests of
qpb_solve_shared / qpb_solve_shared_backward share (tests/test_gpu_shared*.py).

The family: ONE H0 and ONE A0 for the batch, QP 0's of
eq_oracle.eq_family(seed, B, n, m, meq); f and xc per QP from the same call;
b_k = A0 xc_k + slack_k with slack >= 1 on the rows >= meq and 0 on the
equalities, so every QP is strictly feasible by construction.

`shared_backward` calls qpb_solve_shared_backward through the C-ABI into
buffers of its own, filled with 0xA5 and fenced by guard words (the helpers of
tests/bwd_harness.py), and checks that every element was written and nothing
outside.  `sum_bound` is the derived error bound of a summed gradient.
"""
import ctypes
import math

import numpy as np

import eq_oracle as EO
import oracle as O
from bwd_harness import FILL8, GUARD, NAMES, dev

SEED = 11
SHARED_H, SHARED_A = 1, 2
# (n, m, meq): the n < 16 path | n = 16, not FULL | FULL | the wave kernel
DENSE_SHAPES = [(5, 9, 2), (3, 0, 0), (1, 1, 0), (16, 20, 0), (16, 32, 4)]
WAVE_SHAPES = [(16, 33, 0), (17, 34, 3), (20, 40, 4), (32, 64, 8)]
SHAPES = DENSE_SHAPES + WAVE_SHAPES


def batches(qpb):
    """1 and 5 (a ragged MFMA step, a ragged group of four), 67, and a batch of
    two full slices of the sum's plan and a ragged third."""
    slots, per = qpb.sum_plan(2 * qpb.SUM_MIN_SLICE + 37)
    assert slots == 3 and per == qpb.SUM_MIN_SLICE
    return [1, 5, 67, 2 * per + 37]


_FAMILY = {}


def family(B, n, m, meq):
    """(H0 (n,n), f (B,n), A0 (m,n), b (B,m)): computed once, shared, never modified."""
    key = (B, n, m, meq)
    if key not in _FAMILY:
        if m == 0:  # eq_family has no rows to shift: its H and f (family_conditioned's), no A
            H, f, _, _ = O.family_conditioned(SEED, B, n, m=0, box=10.0, kind="dense")
            A, xc = np.zeros((B, 0, n)), np.zeros((B, n))
        else:
            H, f, A, _, xc = EO.eq_family(SEED, B, n, m, meq)
        H0, A0 = np.ascontiguousarray(H[0]), np.ascontiguousarray(A[0])
        slack = np.random.default_rng([SEED, 0x5A, n, m]).uniform(1.0, 10.0, size=(B, m))
        slack[:, :meq] = 0.0
        b = xc @ A0.T + slack
        _FAMILY[key] = (H0, f, A0, b)
    return _FAMILY[key]


def expand(M, B):
    """B materialised copies of a shared matrix."""
    return np.broadcast_to(M, (B,) + M.shape).copy()


def operand(M, B, is_shared):
    return np.ascontiguousarray(M) if is_shared else expand(M, B)


def shared_backward(qpb, shared, H, A, x, lam, act, st, g, need=NAMES, stream=None):
    """qpb_solve_shared_backward through the C-ABI on numpy inputs: H is (n, n)
    with SHARED_H in `shared`, else (B, n, n), and A likewise (st None: status
    NULL).  Returns a dict of the numpy outputs in `need`; a shared operand's
    gradient has the operand's 2-D shape."""
    import torch
    Bq, n = g.shape
    m = A.shape[-2]
    ins = [dev(H), dev(A) if m else None, dev(x), dev(lam) if m else None, dev(act) if m else None,
           dev(st) if st is not None else None, dev(g)]
    shp = {"H": H.shape, "f": (Bq, n), "A": A.shape, "b": (Bq, m)}
    bufs, views = {}, {}
    for k, shape in shp.items():
        if k in need and math.prod(shape) > 0:
            t = torch.empty(math.prod(shape) + 2 * GUARD, dtype=torch.float64, device="cuda")
            t.view(torch.uint8).fill_(0xA5)
            bufs[k], views[k] = t, t[GUARD:GUARD + math.prod(shape)].view(shape)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    d = qpb.Desc(n, m, Bq, 0, 0, 0.0)
    s = stream if stream is not None else torch.cuda.current_stream()
    rc = qpb.lib().qpb_solve_shared_backward(ctypes.byref(d), shared, *[ptr(t) for t in ins],
                                             *[ptr(views.get(k)) for k in NAMES], ctypes.c_void_p(s.cuda_stream))
    assert rc == 0, qpb.lib().qpb_last_error()
    s.synchronize()
    out = {}
    for k, t in bufs.items():
        raw = t.cpu().numpy().view(np.int64)
        assert (raw[:GUARD] == FILL8).all() and (raw[-GUARD:] == FILL8).all(), (k, "guard words written")
        assert not (raw[GUARD:-GUARD] == FILL8).any(), (k, "elements never written")
        out[k] = views[k].cpu().numpy()
    return out


def fsum0(a):
    """The exactly rounded sum over axis 0 (math.fsum per element)."""
    flat = a.reshape(a.shape[0], -1)
    return np.array([math.fsum(flat[:, j]) for j in range(flat.shape[1])]).reshape(a.shape[1:])


def sum_bound(x, gf, gb, lam, mask, ok):
    """(bound_H (n,n), bound_A (m,n)): elementwise (B + 4) 2^-53 T, T the sum
    over the contributing QPs k of the absolute values of the two products of
    each term -- |dx_i x_j| + |x_i dx_j| for gH (twice the 1/2 of each), and
    |dlam_i x_j| + |lam_i dx_j| over the rows in W_k for gA, with dx = gf and
    dlam = -gb.  Any order of B additions of B terms is within (B - 1) u of the
    sum of their absolute values to first order, and each product adds one
    rounding; u = 2^-53.  Derived, not measured."""
    B = x.shape[0]
    xk, dx = np.abs(x[ok]), np.abs(gf[ok])
    TH = 0.5 * (np.einsum("ki,kj->ij", dx, xk) + np.einsum("ki,kj->ij", xk, dx))
    u = (B + 4) * 2.0 ** -53
    if lam.shape[1] == 0:
        return u * TH, np.zeros((0, x.shape[1]))
    lm = np.where(mask[ok], np.abs(lam[ok]), 0.0)
    TA = np.einsum("ki,kj->ij", np.abs(gb[ok]), xk) + np.einsum("ki,kj->ij", lm, dx)
    return u * TH, u * TA
