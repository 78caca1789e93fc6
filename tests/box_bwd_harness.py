"""TEST INFRASTRUCTURE ONLY: what the GPU tests of qpb_solve_box_backward share
(tests/test_gpu_box_backward.py), in tests/bwd_harness.py's manner.

`backward` calls qpb_solve_box_backward through the C-ABI into buffers of its
own, filled with 0xA5 and fenced by guard words, and checks that every element
was written and nothing outside.
"""
import ctypes
import math

import numpy as np

from box_bwd_oracle import NAMES
from bwd_harness import FILL8, GUARD, dev


def shapes(Bq, n):
    return {"H": (Bq, n, n), "f": (Bq, n), "lb": (Bq, n), "ub": (Bq, n)}


def backward(qpb, H, x, act, st, g, need=NAMES, stream=None):
    """qpb_solve_box_backward through the C-ABI on numpy inputs (st None:
    status NULL).  Outputs live between guard words in buffers filled with
    0xA5: every element must have been written and no guard touched.  Returns
    a dict of the numpy arrays in `need`."""
    import torch
    Bq, n = g.shape
    ins = [dev(H), dev(x), dev(act), dev(st) if st is not None else None, dev(g)]
    bufs, views = {}, {}
    for k, shape in shapes(Bq, n).items():
        if k in need:
            t = torch.empty(math.prod(shape) + 2 * GUARD, dtype=torch.float64, device="cuda")
            t.view(torch.uint8).fill_(0xA5)
            bufs[k], views[k] = t, t[GUARD:GUARD + math.prod(shape)].view(shape)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    d = qpb.Desc(n, 2 * n, Bq, 0, 0, 0.0)
    s = stream if stream is not None else torch.cuda.current_stream()
    rc = qpb.lib().qpb_solve_box_backward(ctypes.byref(d), *[ptr(t) for t in ins],
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
