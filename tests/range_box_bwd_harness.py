"""TEST INFRASTRUCTURE ONLY: what the GPU tests of qpb_solve_range_box_backward
share (tests/test_gpu_range_box_backward.py).

`native` calls qpb_solve_range_box_backward through the C-ABI.  Its seven
outputs live side by side in ONE arena filled with a NaN of a payload of its
own, a guard of GUARD doubles before, between and behind them: after the call
every element of a wanted output must have been written, every guard and every
unwanted output's place (its pointer is NULL) must still hold the fill.
`materialised` is the specification: qpb_solve_backward_dual through the C-ABI
on A' = [G; I] built here, its gA cut to the rows of G and its gb routed by the
`lower` bits with numpy.  `same` compares two results bit for bit.
"""
import ctypes
import math

import numpy as np

import range_oracle as RO

GUARD = 64
NAMES = ("H", "f", "G", "bl", "bu", "lb", "ub")
FILL = np.array([0x7FF8A5A5A5A5A5A5], dtype=np.uint64).view(np.int64)[0]  # a quiet NaN no kernel computes


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def out_shapes(H, G, Bq, n, mg):
    return {"H": tuple(H.shape), "f": (Bq, n), "G": tuple(G.shape) if mg else (0,), "bl": (Bq, mg), "bu": (Bq, mg),
            "lb": (Bq, n), "ub": (Bq, n)}


def _ptr(t):
    # (the C ABI reads row-major memory: a tensor that is right only through its strides is a test bug)
    assert t is None or t.is_contiguous(), "a non-contiguous tensor at the C ABI"
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def native(qpb, H, G, x, lam, act, low, st, gx, glam=None, need=NAMES, stream=None):
    """qpb_solve_range_box_backward on device tensors (G, low, st, glam may be
    None; a 2-D H or G is shared).  Returns {name: numpy array} of `need`."""
    import torch
    Bq, n = gx.shape
    mg = 0 if G is None else G.shape[-2]
    shapes = out_shapes(H, G, Bq, n, mg)
    sizes = {k: math.prod(shapes[k]) for k in NAMES}
    arena = torch.empty(GUARD + sum(s + GUARD for s in sizes.values()), dtype=torch.float64, device="cuda")
    arena.view(torch.int64).fill_(int(FILL))
    at, views, off = {}, {}, GUARD
    for k in NAMES:
        at[k] = off
        if k in need and sizes[k]:
            views[k] = arena[off:off + sizes[k]].view(shapes[k])
        off += sizes[k] + GUARD
    shared = (1 if H.dim() == 2 else 0) | (2 if mg and G.dim() == 2 else 0)
    d = qpb.Desc(n, mg, Bq, 0, 0, 0.0)
    s = stream if stream is not None else torch.cuda.current_stream()
    s.wait_stream(torch.cuda.current_stream())  # the fill above
    rc = qpb.lib().qpb_solve_range_box_backward(
        ctypes.byref(d), shared, _ptr(H), _ptr(G), _ptr(x), _ptr(lam), _ptr(act), _ptr(low), _ptr(st), _ptr(gx),
        _ptr(glam), *[_ptr(views.get(k)) for k in NAMES], ctypes.c_void_p(s.cuda_stream))
    assert rc == 0, qpb.lib().qpb_last_error()
    s.synchronize()
    raw = arena.cpu().numpy().view(np.int64)
    assert (raw[:GUARD] == FILL).all(), "the first guard was written"
    out = {}
    for k in NAMES:
        body, guard = raw[at[k]:at[k] + sizes[k]], raw[at[k] + sizes[k]:at[k] + sizes[k] + GUARD]
        assert (guard == FILL).all(), (k, "the guard behind it was written")
        if k in views:
            assert not (body == FILL).any(), (k, "elements never written")
            out[k] = views[k].cpu().numpy()
        else:
            assert (body == FILL).all(), (k, "the place of a NULL output was written")
    return out


def stack(G, Bq, n):
    """A' = [G; I] on the device: (mg + n, n) for a 2-D G, else (B, mg + n, n)."""
    import torch
    eye = torch.eye(n, dtype=torch.float64, device="cuda")
    if G is None:
        return eye.expand(Bq, n, n).contiguous()
    if G.dim() == 2:
        return torch.cat([G, eye], dim=0).contiguous()
    return torch.cat([G, eye.expand(Bq, n, n)], dim=1).contiguous()


def materialised(qpb, H, G, x, lam, act, low, st, gx, glam=None, stream=None):
    """The specification: qpb_solve_backward_dual on [G; I] with all four
    outputs, then the cut and the routing.  Returns all seven names (G: the first
    mg rows of gA') and "A", "b": the call's own gA' and gb'."""
    import torch
    Bq, n = gx.shape
    mg = 0 if G is None else G.shape[-2]
    m = mg + n
    A = stack(G, Bq, n)
    shared = (1 if H.dim() == 2 else 0) | (2 if A.dim() == 2 else 0)
    new = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")  # noqa: E731
    gH, gf, gA, gb = new(*H.shape), new(Bq, n), new(*A.shape), new(Bq, m)
    d = qpb.Desc(n, m, Bq, 0, 0, 0.0)
    s = stream if stream is not None else torch.cuda.current_stream()
    s.wait_stream(torch.cuda.current_stream())  # A' and the fills above
    rc = qpb.lib().qpb_solve_backward_dual(ctypes.byref(d), shared, _ptr(H), _ptr(A), _ptr(x), _ptr(lam), _ptr(act),
                                           _ptr(st), _ptr(gx), _ptr(glam), _ptr(gH), _ptr(gf), _ptr(gA), _ptr(gb),
                                           ctypes.c_void_p(s.cuda_stream))
    assert rc == 0, qpb.lib().qpb_last_error()
    s.synchronize()
    gA, gb = gA.cpu().numpy(), gb.cpu().numpy()
    lo = np.zeros((Bq, m), dtype=bool) if low is None else RO.unpack_bits(low.cpu().numpy().view(np.uint32), m)
    to_lo, to_hi = np.where(lo, gb, 0.0), np.where(lo, 0.0, gb)
    return {"H": gH.cpu().numpy(), "f": gf.cpu().numpy(), "G": np.ascontiguousarray(gA[..., :mg, :]),
            "bl": np.ascontiguousarray(to_lo[:, :mg]), "bu": np.ascontiguousarray(to_hi[:, :mg]),
            "lb": np.ascontiguousarray(to_lo[:, mg:]), "ub": np.ascontiguousarray(to_hi[:, mg:]), "A": gA, "b": gb}


def same(out, ref, names=None):
    """Every array of `out` (or of `names`) equals ref's as int64 bit patterns; an
    output with no element (mg == 0) is absent from `out`."""
    for k in (out.keys() if names is None else names):
        if k not in out:
            assert ref[k].size == 0, k
            continue
        a, b = np.ascontiguousarray(out[k]), np.ascontiguousarray(ref[k])
        assert a.shape == b.shape, (k, a.shape, b.shape)
        if not np.array_equal(a.view(np.int64), b.view(np.int64)):
            bad = np.argwhere(a.view(np.int64) != b.view(np.int64))
            raise AssertionError(f"{k}: {len(bad)} of {a.size} elements differ, first at {bad[0].tolist()}: "
                                 f"{a[tuple(bad[0])]!r} against {b[tuple(bad[0])]!r}")
    return True
