"""TEST INFRASTRUCTURE ONLY: C-ABI callers of qpb_factor_shared_backward and
qpb_solve_factored_backward for tests/test_gpu_factored_backward*.py.

Both write into buffers of their own, filled with 0xA5 and fenced by guard
words (as shared_cases.shared_backward does): every element of every non-NULL
output is written and nothing outside, and the factor buffer is written in
full.  The inputs and the reference are the existing helpers', unchanged.
"""
import ctypes
import math

import numpy as np

from bwd_harness import FILL8, GUARD, NAMES, dev

FILL4 = np.frombuffer(bytes([0xA5] * 4), dtype=np.int32)[0]


def _guarded(torch, count, dt):
    g = GUARD * (2 if dt == torch.int32 else 1)  # GUARD doubles either side
    t = torch.empty(count + 2 * g, dtype=dt, device="cuda")
    t.view(torch.uint8).fill_(0xA5)
    return t, g


def _checked(t, g, name):
    raw = t.cpu().numpy()
    raw, fill = (raw.view(np.int64), FILL8) if raw.dtype == np.float64 else (raw, FILL4)
    assert (raw[:g] == fill).all() and (raw[-g:] == fill).all(), (name, "guard words written")
    assert not (raw[g:-g] == fill).any(), (name, "elements never written")
    return t[g:t.numel() - g].cpu().numpy()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Factor:
    """A backward buffer on the device between guard words, with its fstatus."""

    def __init__(self, n, m, ft, fg, st, sg):
        self.n, self.m, self.ft, self.fg, self.st, self.sg = n, m, ft, fg, st, sg

    @property
    def fac(self):
        """The device view the solve reads (16-byte aligned: GUARD doubles into a torch allocation)."""
        return self.ft[self.fg:self.ft.numel() - self.fg]

    def result(self):
        """(buffer as numpy, fstatus): guards intact, every double and the status written."""
        return _checked(self.ft, self.fg, "bfac"), int(_checked(self.st, self.sg, "fstatus")[0])


def factor(qpb, H0, A0, stream=None, fstatus=True):
    """qpb_factor_shared_backward on numpy H0 (n, n) and A0 (m, n); no host
    synchronisation when `stream` is given: a solve may be queued behind it."""
    import torch
    n, m = H0.shape[0], A0.shape[0]
    k = qpb.lib().qpb_factor_backward_doubles(n, m)
    assert k == qpb.factor_backward_doubles(n, m) and k > 0
    s = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(s):
        ft, fg = _guarded(torch, k, torch.float64)
        st, sg = _guarded(torch, 1, torch.int32)
        H, A = dev(H0), dev(A0) if m else None
    rc = qpb.lib().qpb_factor_shared_backward(n, m, _ptr(H), _ptr(A), _ptr(ft[fg:]), _ptr(st[sg:]) if fstatus else None,
                                              ctypes.c_void_p(s.cuda_stream))
    assert rc == 0, qpb.lib().qpb_last_error()
    if stream is None:
        s.synchronize()
    F = Factor(n, m, ft, fg, st, sg)
    F.keep = (H, A)  # alive until the launch has run
    return F


def factored_backward(qpb, F, x, lam, act, st, g, need=NAMES, stream=None):
    """qpb_solve_factored_backward through the C-ABI on numpy inputs (st None:
    status NULL).  Returns a dict of the numpy outputs in `need`: gH (n, n),
    gf (B, n), gA (m, n), gb (B, m); at m == 0 without A and b."""
    import torch
    Bq, n = g.shape
    m = F.m
    assert n == F.n
    s = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(s):
        ins = [dev(x), dev(lam) if m else None, dev(act) if m else None, dev(st) if st is not None else None, dev(g)]
    shp = {"H": (n, n), "f": (Bq, n), "A": (m, n), "b": (Bq, m)}
    bufs, views = {}, {}
    with torch.cuda.stream(s):  # the fills on the call's stream: no host synchronisation before it
        for k, shape in shp.items():
            if k in need and math.prod(shape) > 0:
                t = torch.empty(math.prod(shape) + 2 * GUARD, dtype=torch.float64, device="cuda")
                t.view(torch.uint8).fill_(0xA5)
                bufs[k], views[k] = t, t[GUARD:GUARD + math.prod(shape)].view(shape)
    d = qpb.Desc(n, m, Bq, 0, 0, 0.0)
    rc = qpb.lib().qpb_solve_factored_backward(ctypes.byref(d), _ptr(F.fac), *[_ptr(t) for t in ins],
                                               *[_ptr(views.get(k)) for k in NAMES], ctypes.c_void_p(s.cuda_stream))
    assert rc == 0, qpb.lib().qpb_last_error()
    s.synchronize()
    out = {}
    for k, t in bufs.items():
        raw = t.cpu().numpy().view(np.int64)
        assert (raw[:GUARD] == FILL8).all() and (raw[-GUARD:] == FILL8).all(), (k, "guard words written")
        assert not (raw[GUARD:-GUARD] == FILL8).any(), (k, "elements never written")
        out[k] = views[k].cpu().numpy()
    return out


def bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def same(got, ref, where):
    assert got.keys() == ref.keys(), (where, sorted(got), sorted(ref))
    for k in got:
        assert bits(got[k], ref[k]), (where, k, "differs from qpb_solve_shared_backward",
                                      float(np.nanmax(np.abs(got[k] - ref[k]))))
