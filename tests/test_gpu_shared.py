"""qpb_solve_shared on the GPU: one H and / or one A for the whole batch, read
from one copy.  The contract is equality bit for bit: x, lam, active, status
and iters of every QP are what qpb_solve_eq writes for it on materialised
copies (np.broadcast_to(...).copy()) -- on the strictly feasible family of
tests/shared_cases.py, and on a batch with mixed statuses (infeasible rows, NaN
entries in b, max_iter = 2).  Every call goes through the C-ABI into buffers
filled with 0xA5 and fenced by guard words (tests/bwd_harness.py's helpers):
every element is written and nothing outside.
"""
import ctypes

import numpy as np
import pytest

import shared_cases as SC
from bwd_harness import FILL8, GUARD, dev as _dev

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

OK = 0
OUT = ("x", "lam", "active", "status", "iters")
FILL4 = np.frombuffer(bytes([0xA5] * 4), dtype=np.int32)[0]


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    return q


def _solve(qpb, shared, H, f, A, b, meq, max_iter=0, stream=None):
    """qpb_solve_shared (shared None: qpb_solve_eq) through the C-ABI on numpy
    inputs, into guarded buffers; a dict of numpy outputs."""
    B, n = f.shape
    m = A.shape[-2]
    w = (m + 31) // 32
    ins = [_dev(H), _dev(f), _dev(A) if m else None, _dev(b) if m else None]
    spec = {"x": (B * n, torch.float64), "lam": (B * m, torch.float64), "active": (B * w, torch.int32),
            "status": (B, torch.int32), "iters": (B, torch.int32)}
    bufs, views = {}, {}
    for k, (count, dt) in spec.items():
        if count:
            g = GUARD * (2 if dt == torch.int32 else 1)  # GUARD doubles either side
            t = torch.empty(count + 2 * g, dtype=dt, device="cuda")
            t.view(torch.uint8).fill_(0xA5)
            bufs[k], views[k] = (t, g), t[g:g + count]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    d = qpb.Desc(n, m, B, max_iter, 0, 0.0)
    s = stream if stream is not None else torch.cuda.current_stream()
    args = [ptr(t) for t in ins] + [ptr(views.get(k)) for k in OUT] + [ctypes.c_void_p(s.cuda_stream)]
    if shared is None:
        rc = qpb.lib().qpb_solve_eq(ctypes.byref(d), meq, *args)
    else:
        rc = qpb.lib().qpb_solve_shared(ctypes.byref(d), meq, shared, *args)
    assert rc == 0, qpb.lib().qpb_last_error()
    s.synchronize()
    out = {}
    for k, (t, g) in bufs.items():
        raw = t.cpu().numpy()
        raw, fill = (raw.view(np.int64), FILL8) if raw.dtype == np.float64 else (raw, FILL4)
        assert (raw[:g] == fill).all() and (raw[-g:] == fill).all(), (k, "guard words written")
        if k != "active":  # (a mask may hold any bits)
            assert not (raw[g:-g] == fill).any(), (k, "elements never written")
        out[k] = views[k].cpu().numpy()
    return out


def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


_REF = {}


def _reference(qpb, B, n, m, meq):
    """qpb_solve_eq on materialised copies: once per case, shared, never modified."""
    key = (B, n, m, meq)
    if key not in _REF:
        H0, f, A0, b = SC.family(B, n, m, meq)
        _REF[key] = _solve(qpb, None, SC.expand(H0, B), f, SC.expand(A0, B), b, meq)
    return _REF[key]


@pytest.mark.parametrize("n,m,meq", SC.SHAPES)
def test_bitwise_equal_to_solve_eq_on_copies(qpb, n, m, meq):
    for B in SC.batches(qpb):
        H0, f, A0, b = SC.family(B, n, m, meq)
        ref = _reference(qpb, B, n, m, meq)
        assert (ref["status"] == OK).all(), (B, ref["status"])
        for shared in (1, 2, 3):
            got = _solve(qpb, shared, SC.operand(H0, B, shared & 1), f, SC.operand(A0, B, shared & 2), b, meq)
            assert _same(got, ref), (B, shared)


def _mixed(B, n, m, meq):
    """The family with its last row the negative of the one before, so that the
    two bound a slab: of width 1 (feasible), empty on every third QP
    (infeasible rows), and with NaN entries in b (absent rows) on every fifth.
    max_iter = 2 caps the rest."""
    H0, f, A0, b = SC.family(B, n, m, meq)
    A0 = A0.copy()
    b = b.copy()
    A0[m - 1] = -A0[m - 2]  # rows m-2 and m-1: a x <= b1 and -a x <= b2, infeasible iff b1 + b2 < 0
    b[:, m - 1] = -b[:, m - 2] + 1.0  # feasible: a slab of width 1 ...
    b[::3, m - 1] = -b[::3, m - 2] - 1.0  # ... and an empty one on every third QP
    b[1::5, meq] = np.nan  # an absent inequality
    return H0, f, A0, b


@pytest.mark.parametrize("n,m,meq", [(5, 9, 2), (16, 20, 0), (16, 32, 4), (20, 40, 4), (32, 64, 8)])
def test_bitwise_equal_on_mixed_statuses(qpb, n, m, meq):
    B = 67
    H0, f, A0, b = _mixed(B, n, m, meq)
    seen = set()
    for max_iter in (0, 2):
        ref = _solve(qpb, None, SC.expand(H0, B), f, SC.expand(A0, B), b, meq, max_iter=max_iter)
        seen |= set(ref["status"].tolist())
        for shared in (1, 2, 3):
            got = _solve(qpb, shared, SC.operand(H0, B, shared & 1), f, SC.operand(A0, B, shared & 2), b, meq,
                         max_iter=max_iter)
            assert _same(got, ref), (max_iter, shared)
    assert {0, 1, 3} <= seen, seen  # OK, MAX_ITER and INFEASIBLE all occurred


def test_nan_inputs_bitwise(qpb):
    """NaN in the shared H (NOT_SPD everywhere) and NaN / Inf in f: the same outputs, status included."""
    n, m, meq, B = 16, 32, 4, 67
    H0, f, A0, b = SC.family(B, n, m, meq)
    f = f.copy()
    f[3, 2] = np.nan
    f[7, 0] = np.inf
    for Hn in (H0, np.where(np.eye(n, dtype=bool) & (np.arange(n) == 5)[:, None], np.nan, H0)):
        ref = _solve(qpb, None, SC.expand(Hn, B), f, SC.expand(A0, B), b, meq)
        got = _solve(qpb, 3, Hn, f, A0, b, meq)
        assert _same(got, ref)
        assert (ref["status"] != OK).any()


@pytest.mark.parametrize("n,m,meq", [(16, 32, 4), (20, 40, 4)])
def test_side_stream_gives_the_same_bits(qpb, n, m, meq):
    B = 67
    H0, f, A0, b = SC.family(B, n, m, meq)
    ref = _reference(qpb, B, n, m, meq)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    got = _solve(qpb, 3, H0, f, A0, b, meq, stream=side)
    assert _same(got, ref)


def test_shared_zero_is_solve_eq(qpb):
    n, m, meq, B = 16, 32, 4, 67
    H0, f, A0, b = SC.family(B, n, m, meq)
    got = _solve(qpb, 0, SC.expand(H0, B), f, SC.expand(A0, B), b, meq)
    assert _same(got, _reference(qpb, B, n, m, meq))


def test_python_call_and_unsupported_above_the_wave_classes(qpb):
    n, m, meq, B = 16, 32, 4, 5
    H0, f, A0, b = SC.family(B, n, m, meq)
    sol = qpb.solve_shared(_dev(H0), _dev(f), _dev(A0), _dev(b), meq)
    torch.cuda.synchronize()
    ref = _reference(qpb, B, n, m, meq)
    assert np.array_equal(sol.x.cpu().numpy().ravel(), ref["x"])
    assert np.array_equal(sol.status.cpu().numpy(), ref["status"])
    # batched 3-D operands through the same call
    sol = qpb.solve_shared(_dev(SC.expand(H0, B)), _dev(f), _dev(A0), _dev(b), meq)
    torch.cuda.synchronize()
    assert np.array_equal(sol.x.cpu().numpy().ravel(), ref["x"])
    for n, m in ((33, 40), (32, 65), (48, 0)):
        H = torch.eye(n, dtype=torch.float64, device="cuda")
        f = torch.zeros((4, n), dtype=torch.float64, device="cuda")
        A = torch.zeros((m, n), dtype=torch.float64, device="cuda") if m else None
        bb = torch.zeros((4, m), dtype=torch.float64, device="cuda") if m else None
        with pytest.raises(qpb.QPBError) as e:
            qpb.solve_shared(H, f, A, bb)
        assert e.value.code == qpb.ERR_UNSUPPORTED and "shared" in str(e.value)
    # with nothing shared the same shape is qpb_solve_eq's: the Gram class solves it
    H = torch.eye(48, dtype=torch.float64, device="cuda").expand(4, 48, 48).contiguous()
    sol = qpb.solve_shared(H, torch.ones((4, 48), dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    assert (sol.status.cpu().numpy() == OK).all()
    assert np.allclose(sol.x.cpu().numpy(), -1.0)
