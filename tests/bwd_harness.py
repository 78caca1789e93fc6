"""TEST INFRASTRUCTURE ONLY: what the GPU tests of qpb_solve_backward share
(tests/test_gpu_backward.py, tests/test_gpu_backward_edges.py).

`backward` calls qpb_solve_backward through the C-ABI into buffers of its own,
filled with 0xA5 and fenced by guard words, and checks that every element was
written and nothing outside.  `same` compares two results bit for bit, `rel`
is the project's error measure.  torch is imported by the calls that need a
device only, so the CPU tests can use `rel` and the bars.
"""
import ctypes
import math

import numpy as np

X_TOL = 1e-6
KKT_TOL = 1e-9
GUARD = 64  # doubles on either side of an output
NAMES = ("H", "f", "A", "b")

FILL8 = np.frombuffer(bytes([0xA5] * 8), dtype=np.int64)[0]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def shapes(Bq, n, m):
    return {"H": (Bq, n, n), "f": (Bq, n), "A": (Bq, m, n), "b": (Bq, m)}


def backward(qpb, H, A, x, lam, act, st, g, need=NAMES, stream=None):
    """qpb_solve_backward through the C-ABI on numpy inputs (st None: status
    NULL).  Outputs live between guard words in buffers filled with 0xA5: every
    element must have been written and no guard touched.  Returns a dict of the
    numpy arrays in `need` (at m == 0 without A and b)."""
    import torch
    Bq, n = g.shape
    m = A.shape[1]
    ins = [dev(H), dev(A) if m else None, dev(x), dev(lam) if m else None, dev(act) if m else None,
           dev(st) if st is not None else None, dev(g)]
    bufs, views = {}, {}
    for k, shape in shapes(Bq, n, m).items():
        if k in need and math.prod(shape) > 0:
            t = torch.empty(math.prod(shape) + 2 * GUARD, dtype=torch.float64, device="cuda")
            t.view(torch.uint8).fill_(0xA5)
            bufs[k], views[k] = t, t[GUARD:GUARD + math.prod(shape)].view(shape)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    d = qpb.Desc(n, m, Bq, 0, 0, 0.0)
    s = stream if stream is not None else torch.cuda.current_stream()
    rc = qpb.lib().qpb_solve_backward(ctypes.byref(d), *[ptr(t) for t in ins], *[ptr(views.get(k)) for k in NAMES],
                                      ctypes.c_void_p(s.cuda_stream))
    assert rc == 0, qpb.lib().qpb_last_error()
    s.synchronize()
    out = {}
    for k, t in bufs.items():
        raw = t.cpu().numpy().view(np.int64)
        assert (raw[:GUARD] == FILL8).all() and (raw[-GUARD:] == FILL8).all(), (k, "guard words written")
        assert not (raw[GUARD:-GUARD] == FILL8).any(), (k, "elements never written")
        out[k] = views[k].cpu().numpy()
    return out


def same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


def rel(a, ref):
    """max|delta| / (1 + max|ref|) per QP."""
    ax = tuple(range(1, a.ndim))
    return np.abs(a - ref).max(axis=ax) / (1.0 + np.abs(ref).max(axis=ax))
