"""qpb.diff -- the solver as a differentiable torch function.

``solve(H, f, A, b, meq)`` is ``qpb.solve_eq`` with gradients: the backward
pass is ``qpb.solve_backward`` (qpb_solve_backward, one KKT solve per QP at the
solution's active set, on the GPU).  This module imports torch at the top;
``import qpb`` itself stays torch-free.

    x, status = qpb.diff.solve(H, f, A, b, meq=2)   # H, f, A, b may require grad
    loss = (w * x).sum()
    loss.backward()                                 # H.grad, f.grad, A.grad, b.grad

A 2-D ``H`` (n, n) and / or ``A`` (m, n) is ONE matrix for the whole batch --
the weights of a QP layer, with f and b from the network's input: the solve is
``qpb.solve_shared``, the backward ``qpb.solve_shared_backward``, ``H.grad``
is (n, n), and no (B, n, n) or (B, m, n) tensor is ever allocated.  With
``prefactor=True`` (a 2-D H and, when there are rows, a 2-D A) the forward
factors the two once, ``qpb.factor_shared``, and solves with
``qpb.solve_factored``, and the backward factors the saved H and A once,
``qpb.factor_shared_backward``, and runs ``qpb.solve_factored_backward``: the
per-QP set-up is gone from both passes.  The gradients are bit for bit those of
``qpb.solve_shared_backward``; a forward without gradients pays nothing for them.

``solve_box(H, f, lb, ub)`` is ``qpb.solve_box`` with gradients for H, f, lb
and ub (``qpb.solve_box_backward``, n <= 32).  A 2-D ``H`` (n, n) is ONE matrix
for the whole batch there as well: the solve is ``qpb.solve_box_shared``, the
backward ``qpb.solve_box_shared_backward``, ``H.grad`` is (n, n) -- the sum over
the batch -- and no (B, n, n) tensor is allocated in either pass.  With
``prefactor=True`` (a 2-D H, n <= 32) the forward factors H once,
``qpb.factor_box``, and solves with ``qpb.solve_box_factored``; the backward is
``qpb.solve_box_shared_backward`` on the saved H, unchanged.

``solve_range(H, f, A, bl, bu, meq)`` is ``qpb.solve_range`` with gradients for
H, f, A, bl and bu: the backward is ``qpb.solve_backward`` (or the shared one)
on the range solve's outputs, its ``gb`` routed to ``bl`` or ``bu`` by the
``lower`` bits.  ``prefactor=True`` (a 2-D H and a 2-D A) factors once per
forward and solves with ``qpb.solve_range_factored``; the backward is the
factored one in the same way.

``solve_range_box(H, f, G, bl, bu, lb, ub, meq)`` is ``qpb.solve_range_box`` --
those rows beside variable bounds, no identity rows in G -- with gradients for
H, f, G and the four bounds.  The backward is ``qpb.solve_range_box_backward``:
neither pass builds ``[G; I]``, and the gradients are bit for bit those of
``qpb.solve_backward`` (or the shared one) on it.  ``solve_range_box_dual``
returns ``(x, lam, status)`` with lam differentiable as well, in the manner of
``solve_range_dual``.

``solve_dual(H, f, A, b, meq)`` and ``solve_range_dual(H, f, A, bl, bu, meq)``
return ``(x, lam, status)`` with x AND lam differentiable: the backward is
``qpb.solve_backward_dual`` (qpb_solve_backward_dual, the same KKT system with
the cotangent on lam as its lower right-hand side).  A loss that does not read
lam takes the backward of ``solve`` / ``solve_range``, bit for bit.  With
``prefactor=True`` (a 2-D H and a 2-D A) both passes run on factor buffers as
in ``solve`` / ``solve_range``, the backward by
``qpb.solve_factored_backward_dual``, with the default's gradients bit for bit.

``solve_box_dual(H, f, lb, ub)`` is the same for box QPs: ``(x, lam, status)``
with lam (B, 2n) in ``qpb.solve_box``'s layout, the backward
``qpb.solve_box_backward_dual``; H 2-D or 3-D and ``prefactor`` as in
``solve_box``.
"""
from __future__ import annotations

import torch

import qpb


def _backward(ctx, H, A, sol, gx, wanted):
    """The backward call of a forward: on a prefactored forward the saved H and A
    are factored once for the backward and neither is read per QP."""
    if ctx.prefactor:
        return qpb.solve_factored_backward(qpb.factor_shared_backward(H, A), sol, gx, need=wanted)
    backward = qpb.solve_shared_backward if ctx.shared else qpb.solve_backward
    return backward(H, A, sol, gx, need=wanted)


class QPFunction(torch.autograd.Function):
    """x*(H, f, A, b) of min 1/2 x'Hx + f'x s.t. A[:meq] x = b[:meq], A[meq:] x <= b[meq:]."""

    @staticmethod
    def forward(ctx, H, f, A, b, meq, max_iter, feas_tol, prefactor):
        H, f = H.contiguous(), f.contiguous()
        if A is not None:
            A, b = A.contiguous(), b.contiguous()
        ctx.shared = H.dim() == 2 or (A is not None and A.dim() == 2)
        if prefactor:
            sol = qpb.solve_factored(qpb.factor_shared(H, A), f, b, meq, max_iter=max_iter, feas_tol=feas_tol)
        elif ctx.shared:
            sol = qpb.solve_shared(H, f, A, b, meq, max_iter=max_iter, feas_tol=feas_tol)
        else:
            sol = qpb.solve_eq(H, f, A, b, meq, max_iter=max_iter, feas_tol=feas_tol) if A is not None \
                else qpb.solve(H, f, max_iter=max_iter, feas_tol=feas_tol)
        ctx.has_rows = A is not None
        ctx.prefactor = prefactor
        ctx.save_for_backward(H, A, sol.x, sol.lam, sol.active, sol.status)
        ctx.mark_non_differentiable(sol.status)
        return sol.x, sol.status

    @staticmethod
    def backward(ctx, gx, _gstatus):
        H, A, x, lam, active, status = ctx.saved_tensors
        wanted = [k for k, w in zip("HfAb", ctx.needs_input_grad[:4]) if w and (ctx.has_rows or k in "Hf")]
        if not wanted:
            return (None,) * 8
        sol = qpb.Solution(x, lam, active, status, None)
        # on torch's current stream; above n = 32 or m = 64 this raises QPBError(ERR_UNSUPPORTED)
        gH, gf, gA, gb = _backward(ctx, H, A, sol, gx.contiguous(), wanted)
        return gH, gf, gA, gb, None, None, None, None


class BoxQPFunction(torch.autograd.Function):
    """x*(H, f, lb, ub) of min 1/2 x'Hx + f'x s.t. lb <= x <= ub."""

    @staticmethod
    def forward(ctx, H, f, lb, ub, max_iter, feas_tol, prefactor=False):
        H, f = H.contiguous(), f.contiguous()
        lb = None if lb is None else lb.contiguous()
        ub = None if ub is None else ub.contiguous()
        ctx.shared = H.dim() == 2  # one H for the batch
        if prefactor:
            # above n = 32 this raises QPBError(ERR_UNSUPPORTED)
            sol = qpb.solve_box_factored(qpb.factor_box(H), f, lb, ub, max_iter=max_iter, feas_tol=feas_tol)
        else:
            forward = qpb.solve_box_shared if ctx.shared else qpb.solve_box
            sol = forward(H, f, lb, ub, max_iter=max_iter, feas_tol=feas_tol)
        ctx.has = (True, True, lb is not None, ub is not None)
        ctx.save_for_backward(H, sol.x, sol.active, sol.status)
        ctx.mark_non_differentiable(sol.status)
        return sol.x, sol.status

    @staticmethod
    def backward(ctx, gx, _gstatus):
        H, x, active, status = ctx.saved_tensors
        names = ("H", "f", "lb", "ub")
        wanted = [k for k, w, has in zip(names, ctx.needs_input_grad[:4], ctx.has) if w and has]
        if not wanted:
            return (None,) * 7
        sol = qpb.Solution(x, None, active, status, None)
        # on torch's current stream; above n = 32 this raises QPBError(ERR_UNSUPPORTED)
        backward = qpb.solve_box_shared_backward if ctx.shared else qpb.solve_box_backward
        gH, gf, glb, gub = backward(H, sol, gx.contiguous(), need=wanted)
        return gH, gf, glb, gub, None, None, None


class RangeQPFunction(torch.autograd.Function):
    """x*(H, f, A, bl, bu) of min 1/2 x'Hx + f'x s.t. A[:meq] x = bu[:meq], bl[meq:] <= A[meq:] x <= bu[meq:]."""

    @staticmethod
    def forward(ctx, H, f, A, bl, bu, meq, max_iter, feas_tol, prefactor):
        H, f, A = H.contiguous(), f.contiguous(), A.contiguous()
        bl = None if bl is None else bl.contiguous()
        bu = None if bu is None else bu.contiguous()
        # above n = 32 or m = 64 this raises QPBError(ERR_UNSUPPORTED)
        if prefactor:
            sol = qpb.solve_range_factored(qpb.factor_shared(H, A), f, bl, bu, meq, max_iter=max_iter,
                                           feas_tol=feas_tol)
        else:
            sol = qpb.solve_range(H, f, A, bl, bu, meq, max_iter=max_iter, feas_tol=feas_tol)
        ctx.shared = H.dim() == 2 or A.dim() == 2
        ctx.prefactor = prefactor
        ctx.meq = meq
        ctx.has = (True, True, True, bl is not None, bu is not None)
        ctx.save_for_backward(H, A, sol.x, sol.lam, sol.active, sol.lower, sol.status)
        ctx.mark_non_differentiable(sol.status)
        return sol.x, sol.status

    @staticmethod
    def backward(ctx, gx, _gstatus):
        H, A, x, lam, active, lower, status = ctx.saved_tensors
        want = [w and has for w, has in zip(ctx.needs_input_grad[:5], ctx.has)]
        wanted = [k for k, w in zip("HfA", want[:3]) if w] + (["b"] if want[3] or want[4] else [])
        if not wanted:
            return (None,) * 9
        sol = qpb.Solution(x, lam, active, status, None)
        gH, gf, gA, gb = _backward(ctx, H, A, sol, gx.contiguous(), wanted)
        gbl = gbu = None
        if gb is not None:
            # every element of gb goes to the bound its row is active at: bl where the
            # `lower` bit is set (never on an equality), bu everywhere else
            m = gb.shape[1]
            rows = torch.arange(m, device=gb.device)
            low = ((lower[:, rows // 32] >> (rows % 32)) & 1).bool()
            zero = torch.zeros_like(gb)
            if want[3]:
                gbl = torch.where(low, gb, zero)
            if want[4]:
                gbu = torch.where(low, zero, gb)
        return gH, gf, gA, gbl, gbu, None, None, None, None


class RangeBoxQPFunction(torch.autograd.Function):
    """x*(H, f, G, bl, bu, lb, ub) of min 1/2 x'Hx + f'x s.t. G[:meq] x = bu[:meq],
    bl[meq:] <= G[meq:] x <= bu[meq:], lb <= x <= ub."""

    @staticmethod
    def forward(ctx, H, f, G, bl, bu, lb, ub, meq, max_iter, feas_tol):
        c = lambda t: None if t is None else t.contiguous()  # noqa: E731
        H, f, G, bl, bu, lb, ub = (c(t) for t in (H, f, G, bl, bu, lb, ub))
        # above n = 32 or mg + n = 64 this raises QPBError(ERR_UNSUPPORTED)
        sol = qpb.solve_range_box(H, f, G, bl, bu, lb, ub, meq, max_iter=max_iter, feas_tol=feas_tol)
        ctx.has = (True, True, G is not None) + tuple(t is not None for t in (bl, bu, lb, ub))
        ctx.save_for_backward(H, G, sol.x, sol.lam, sol.active, sol.lower, sol.status)
        ctx.mark_non_differentiable(sol.status)
        return sol.x, sol.status

    @staticmethod
    def backward(ctx, gx, _gstatus):
        grads = _range_box_backward(ctx, gx, None)
        return (None,) * 10 if grads is None else grads + (None, None, None)


_RANGE_BOX_NAMES = ("H", "f", "G", "bl", "bu", "lb", "ub")


def _range_box_backward(ctx, gx, glam):
    """The seven gradients of a range-box forward (None where not wanted), or None
    when none is: ``qpb.solve_range_box_backward`` on the saved solve, on torch's
    current stream.  An unused lam arrives as None and takes the call without
    glam, an unused x is a zero cotangent."""
    H, G, x, lam, active, lower, status = ctx.saved_tensors
    wanted = [k for k, w, has in zip(_RANGE_BOX_NAMES, ctx.needs_input_grad[:7], ctx.has) if w and has]
    if not wanted or (gx is None and glam is None):
        return None
    sol = qpb.RangeSolution(x, lam, active, lower, status, None)
    gx = torch.zeros_like(x) if gx is None else gx.contiguous()
    return qpb.solve_range_box_backward(H, G, sol, gx, None if glam is None else glam.contiguous(), need=wanted)


class RangeBoxDualQPFunction(torch.autograd.Function):
    """(x*, lam*)(H, f, G, bl, bu, lb, ub) of ``RangeBoxQPFunction``'s problem, lam signed, (B, mg + n)."""

    @staticmethod
    def forward(ctx, H, f, G, bl, bu, lb, ub, meq, max_iter, feas_tol):
        c = lambda t: None if t is None else t.contiguous()  # noqa: E731
        H, f, G, bl, bu, lb, ub = (c(t) for t in (H, f, G, bl, bu, lb, ub))
        # above n = 32 or mg + n = 64 this raises QPBError(ERR_UNSUPPORTED)
        sol = qpb.solve_range_box(H, f, G, bl, bu, lb, ub, meq, max_iter=max_iter, feas_tol=feas_tol)
        ctx.has = (True, True, G is not None) + tuple(t is not None for t in (bl, bu, lb, ub))
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(H, G, sol.x, sol.lam, sol.active, sol.lower, sol.status)
        ctx.mark_non_differentiable(sol.status)
        return sol.x, sol.lam, sol.status

    @staticmethod
    def backward(ctx, gx, glam, _gstatus):
        grads = _range_box_backward(ctx, gx, glam)
        return (None,) * 10 if grads is None else grads + (None, None, None)


def _backward_dual(ctx, H, A, x, lam, active, status, gx, glam, wanted):
    """The backward call of the forms that return lam: an unused lam arrives as
    None and takes ``solve_backward``'s kernels, an unused x is a zero cotangent."""
    sol = qpb.Solution(x, lam, active, status, None)
    gx = torch.zeros_like(x) if gx is None else gx.contiguous()
    if glam is None:
        return _backward(ctx, H, A, sol, gx, wanted)
    # on torch's current stream; above n = 32 or m = 64 this raises QPBError(ERR_UNSUPPORTED)
    if ctx.prefactor:
        return qpb.solve_factored_backward_dual(qpb.factor_shared_backward(H, A), sol, gx, glam.contiguous(),
                                                need=wanted)
    return qpb.solve_backward_dual(H, A, sol, gx, glam.contiguous(), need=wanted)


class DualQPFunction(torch.autograd.Function):
    """(x*, lam*)(H, f, A, b) of min 1/2 x'Hx + f'x s.t. A[:meq] x = b[:meq], A[meq:] x <= b[meq:]."""

    @staticmethod
    def forward(ctx, H, f, A, b, meq, max_iter, feas_tol, prefactor=False):
        H, f, A, b = H.contiguous(), f.contiguous(), A.contiguous(), b.contiguous()
        ctx.shared = H.dim() == 2 or A.dim() == 2
        ctx.prefactor = prefactor
        if prefactor:
            sol = qpb.solve_factored(qpb.factor_shared(H, A), f, b, meq, max_iter=max_iter, feas_tol=feas_tol)
        elif ctx.shared:
            sol = qpb.solve_shared(H, f, A, b, meq, max_iter=max_iter, feas_tol=feas_tol)
        else:
            sol = qpb.solve_eq(H, f, A, b, meq, max_iter=max_iter, feas_tol=feas_tol)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(H, A, sol.x, sol.lam, sol.active, sol.status)
        ctx.mark_non_differentiable(sol.status)
        return sol.x, sol.lam, sol.status

    @staticmethod
    def backward(ctx, gx, glam, _gstatus):
        H, A, x, lam, active, status = ctx.saved_tensors
        wanted = [k for k, w in zip("HfAb", ctx.needs_input_grad[:4]) if w]
        if not wanted or (gx is None and glam is None):
            return (None,) * 8
        gH, gf, gA, gb = _backward_dual(ctx, H, A, x, lam, active, status, gx, glam, wanted)
        return gH, gf, gA, gb, None, None, None, None


class RangeDualQPFunction(torch.autograd.Function):
    """(x*, lam*)(H, f, A, bl, bu) of ``RangeQPFunction``'s problem, lam signed."""

    @staticmethod
    def forward(ctx, H, f, A, bl, bu, meq, max_iter, feas_tol, prefactor=False):
        H, f, A = H.contiguous(), f.contiguous(), A.contiguous()
        bl = None if bl is None else bl.contiguous()
        bu = None if bu is None else bu.contiguous()
        # above n = 32 or m = 64 this raises QPBError(ERR_UNSUPPORTED)
        if prefactor:
            sol = qpb.solve_range_factored(qpb.factor_shared(H, A), f, bl, bu, meq, max_iter=max_iter,
                                           feas_tol=feas_tol)
        else:
            sol = qpb.solve_range(H, f, A, bl, bu, meq, max_iter=max_iter, feas_tol=feas_tol)
        ctx.shared = H.dim() == 2 or A.dim() == 2
        ctx.prefactor = prefactor
        ctx.has = (True, True, True, bl is not None, bu is not None)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(H, A, sol.x, sol.lam, sol.active, sol.lower, sol.status)
        ctx.mark_non_differentiable(sol.status)
        return sol.x, sol.lam, sol.status

    @staticmethod
    def backward(ctx, gx, glam, _gstatus):
        H, A, x, lam, active, lower, status = ctx.saved_tensors
        want = [w and has for w, has in zip(ctx.needs_input_grad[:5], ctx.has)]
        wanted = [k for k, w in zip("HfA", want[:3]) if w] + (["b"] if want[3] or want[4] else [])
        if not wanted or (gx is None and glam is None):
            return (None,) * 9
        gH, gf, gA, gb = _backward_dual(ctx, H, A, x, lam, active, status, gx, glam, wanted)
        gbl = gbu = None
        if gb is not None:
            # as in RangeQPFunction: bl where the `lower` bit is set, bu everywhere else
            m = gb.shape[1]
            rows = torch.arange(m, device=gb.device)
            low = ((lower[:, rows // 32] >> (rows % 32)) & 1).bool()
            zero = torch.zeros_like(gb)
            if want[3]:
                gbl = torch.where(low, gb, zero)
            if want[4]:
                gbu = torch.where(low, zero, gb)
        return gH, gf, gA, gbl, gbu, None, None, None, None


class BoxDualQPFunction(torch.autograd.Function):
    """(x*, lam*)(H, f, lb, ub) of ``BoxQPFunction``'s problem, lam (B, 2n): the upper bounds' entries, then the
    lower bounds'."""

    @staticmethod
    def forward(ctx, H, f, lb, ub, max_iter, feas_tol, prefactor):
        H, f = H.contiguous(), f.contiguous()
        lb = None if lb is None else lb.contiguous()
        ub = None if ub is None else ub.contiguous()
        ctx.shared = H.dim() == 2  # one H for the batch
        if prefactor:
            # above n = 32 this raises QPBError(ERR_UNSUPPORTED)
            sol = qpb.solve_box_factored(qpb.factor_box(H), f, lb, ub, max_iter=max_iter, feas_tol=feas_tol)
        else:
            forward = qpb.solve_box_shared if ctx.shared else qpb.solve_box
            sol = forward(H, f, lb, ub, max_iter=max_iter, feas_tol=feas_tol)
        ctx.has = (True, True, lb is not None, ub is not None)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(H, sol.x, sol.active, sol.status)
        ctx.mark_non_differentiable(sol.status)
        return sol.x, sol.lam, sol.status

    @staticmethod
    def backward(ctx, gx, glam, _gstatus):
        H, x, active, status = ctx.saved_tensors
        names = ("H", "f", "lb", "ub")
        wanted = [k for k, w, has in zip(names, ctx.needs_input_grad[:4], ctx.has) if w and has]
        if not wanted or (gx is None and glam is None):
            return (None,) * 7
        sol = qpb.Solution(x, None, active, status, None)
        gx = torch.zeros_like(x) if gx is None else gx.contiguous()
        # on torch's current stream; above n = 32 this raises QPBError(ERR_UNSUPPORTED).  An unused lam
        # arrives as None and takes solve_box's backward.
        gH, gf, glb, gub = qpb.solve_box_backward_dual(H, sol, gx, None if glam is None else glam.contiguous(),
                                                       need=wanted)
        return gH, gf, glb, gub, None, None, None


def solve_box_dual(H, f, lb=None, ub=None, *, max_iter: int = 0, feas_tol: float = 0.0, prefactor: bool = False):
    """``solve_box`` that also returns the multipliers, differentiably: returns
    ``(x, lam, status)`` with ``lam`` (B, 2n) in ``qpb.solve_box``'s layout, the
    upper bounds' entries first; ``x`` and ``lam`` both carry gradients to
    whichever of H, f, lb and ub require them.  The backward is
    ``qpb.solve_box_backward_dual`` on the two cotangents at fixed active set; a
    loss that does not read ``lam`` gets ``solve_box``'s gradients bit for bit,
    and one that does not read ``x`` has gx = 0.  H 2-D (one matrix, its
    gradient the sum over the batch) or 3-D, and ``prefactor``, as in
    ``solve_box``.  The backward needs n <= 32."""
    if prefactor:
        if H.dim() != 2:
            raise ValueError("prefactor=True needs a 2-D H (n, n): one matrix for the batch")
    return BoxDualQPFunction.apply(H, f, lb, ub, int(max_iter), float(feas_tol), bool(prefactor))


def solve_dual(H, f, A, b, meq: int = 0, *, max_iter: int = 0, feas_tol: float = 0.0, prefactor: bool = False):
    """``solve`` that also returns the multipliers, differentiably: returns
    ``(x, lam, status)``; ``x`` and ``lam`` (B, m, H x + f + A' lam = 0) both carry
    gradients to whichever of H, f, A and b require them -- shadow prices,
    constraint-tightness penalties and dual objectives can enter the loss.  The
    backward is ``qpb.solve_backward_dual`` on the two cotangents at fixed active
    set; a loss that does not read ``lam`` runs ``solve``'s backward, bit for
    bit, and one that does not read ``x`` has gx = 0.  A 2-D H (n, n) and / or A
    (m, n) is shared by the batch, its gradient the sum over the batch.  QPs whose
    status is not OK contribute zero gradients.  n <= 32 and m <= 64 in the
    backward (``QPBError(ERR_UNSUPPORTED)`` above).  A is required (without rows
    there is no lam: use ``solve``).  ``prefactor=True`` needs a 2-D H and a 2-D
    A, else ValueError: the forward is ``solve``'s prefactored one, and the
    backward factors H and A once (``qpb.factor_shared_backward``) and runs
    ``qpb.solve_factored_backward_dual``, with the default's gradients bit for
    bit.  The default is today's call, bit for bit."""
    if A is None or b is None:
        raise ValueError("qpb.diff.solve_dual needs A and b: without rows there are no multipliers (use solve)")
    if prefactor:
        if H.dim() != 2 or A.dim() != 2:
            raise ValueError("prefactor=True needs a 2-D H (n, n) and a 2-D A (m, n): one matrix for the batch")
    return DualQPFunction.apply(H, f, A, b, int(meq), int(max_iter), float(feas_tol), bool(prefactor))


def solve_range_dual(H, f, A, bl, bu, meq: int = 0, *, max_iter: int = 0, feas_tol: float = 0.0,
                     prefactor: bool = False):
    """``solve_range`` that also returns the signed multipliers, differentiably:
    returns ``(x, lam, status)`` with ``lam`` in ``qpb.solve_range``'s convention
    (H x + f + A' lam = 0: >= 0 on a row active at bu, <= 0 at bl).  The backward
    is ``qpb.solve_backward_dual`` on the two cotangents; its ``gb`` goes to
    ``bl`` where the ``lower`` bit is set and to ``bu`` everywhere else, exactly
    as in ``solve_range``.  A bound passed as None gets no gradient.  A loss that
    does not read ``lam`` gets ``solve_range``'s gradients bit for bit.  n <= 32
    and m <= 64.  ``prefactor=True`` (a 2-D H and a 2-D A, else ValueError) is
    ``solve_range``'s prefactored forward and ``qpb.solve_factored_backward_dual``
    in the backward, with the default's gradients bit for bit."""
    if prefactor:
        if H.dim() != 2 or A.dim() != 2:
            raise ValueError("prefactor=True needs a 2-D H (n, n) and a 2-D A (m, n): one matrix for the batch")
    return RangeDualQPFunction.apply(H, f, A, bl, bu, int(meq), int(max_iter), float(feas_tol), bool(prefactor))


def solve_range(H, f, A, bl, bu, meq: int = 0, *, max_iter: int = 0, feas_tol: float = 0.0,
                prefactor: bool = False):
    """Differentiable batched solve with two-sided rows (``qpb.solve_range`` with
    gradients): returns ``(x, status)``; ``x`` carries gradients to whichever of
    H, f, A, bl and bu require them.  The backward is ``qpb.solve_backward`` (with
    a 2-D H or A, ``qpb.solve_shared_backward``) on the solve's x, signed lam,
    active and status; its ``gb`` goes to ``bu`` on the rows < meq and on the
    rows active at their upper bound, to ``bl`` on the rows whose ``lower`` bit
    is set.  A bound passed as None gets no gradient.  n <= 32 and m <= 64: above
    that the forward raises ``QPBError(ERR_UNSUPPORTED)``.  ``prefactor=True``
    needs a 2-D H and a 2-D A, else ValueError: the forward factors them once
    (``qpb.factor_shared``) and solves with ``qpb.solve_range_factored``, whose
    x may differ from the default's by rounding; the backward factors H and A
    once (``qpb.factor_shared_backward``) and runs ``qpb.solve_factored_backward``,
    bit for bit ``qpb.solve_shared_backward`` on H and A.  The default is today's
    call, bit for bit."""
    if prefactor:
        if H.dim() != 2 or A.dim() != 2:
            raise ValueError("prefactor=True needs a 2-D H (n, n) and a 2-D A (m, n): one matrix for the batch")
    return RangeQPFunction.apply(H, f, A, bl, bu, int(meq), int(max_iter), float(feas_tol), bool(prefactor))


def solve_range_box(H, f, G, bl, bu, lb=None, ub=None, meq: int = 0, *, max_iter: int = 0, feas_tol: float = 0.0):
    """Differentiable batched solve with two-sided rows beside variable bounds
    (``qpb.solve_range_box`` with gradients): returns ``(x, status)``; ``x``
    carries gradients to whichever of H, f, G, bl, bu, lb and ub require them.
    Neither pass builds ``[G; I]``: the backward is
    ``qpb.solve_range_box_backward``, bit for bit ``qpb.solve_backward``
    (``qpb.solve_shared_backward`` with a 2-D H or G) on it -- ``G.grad`` is its
    first mg rows (one summed (mg, n) matrix for a 2-D G), and its ``gb`` goes to
    ``bl`` / ``bu`` / ``lb`` / ``ub`` by the ``lower`` bits exactly as
    ``solve_range`` routes it.  A bound passed as None gets no gradient.
    n <= 32 and mg + n <= 64: above that the forward raises
    ``QPBError(ERR_UNSUPPORTED)``."""
    return RangeBoxQPFunction.apply(H, f, G, bl, bu, lb, ub, int(meq), int(max_iter), float(feas_tol))


def solve_range_box_dual(H, f, G, bl, bu, lb=None, ub=None, meq: int = 0, *, max_iter: int = 0,
                         feas_tol: float = 0.0):
    """``solve_range_box`` that also returns the signed multipliers,
    differentiably: returns ``(x, lam, status)`` with ``lam`` (B, mg + n) in
    ``qpb.solve_range_box``'s layout and convention (the rows first, then variable
    j at mg + j; >= 0 at an upper bound, <= 0 at a lower one).  The backward is
    ``qpb.solve_range_box_backward`` on the two cotangents, routed to the four
    bounds exactly as in ``solve_range_box``.  A bound passed as None gets no
    gradient.  A loss that does not read ``lam`` gets ``solve_range_box``'s
    gradients bit for bit, and one that does not read ``x`` has gx = 0.
    n <= 32 and mg + n <= 64."""
    return RangeBoxDualQPFunction.apply(H, f, G, bl, bu, lb, ub, int(meq), int(max_iter), float(feas_tol))


def solve_box(H, f, lb=None, ub=None, *, max_iter: int = 0, feas_tol: float = 0.0, prefactor: bool = False):
    """Differentiable batched box solve (``qpb.solve_box`` with gradients):
    returns ``(x, status)``; ``x`` carries gradients to whichever of H, f, lb
    and ub require them, ``status`` (int32 per QP) is not differentiable.  A
    bound passed as None gets no gradient.  QPs whose status is not OK
    contribute zero gradients.  The gradient is the derivative at fixed active
    set (qpb.h, qpb_solve_box_backward).  The forward solves every shape
    ``qpb.solve_box`` does (n <= 128); the backward needs n <= 32 and raises
    ``QPBError(ERR_UNSUPPORTED)`` above that.  H may be 2-D, (n, n): one matrix
    shared by the batch (``qpb.solve_box_shared``, with x bit for bit that of B
    copies), whose gradient (n, n) is the sum over the batch
    (``qpb.solve_box_shared_backward``), computed without a per-QP matrix; a
    3-D H is the batched path unchanged.  ``prefactor=True`` needs a 2-D H, else
    ValueError, and n <= 32 (``QPBError(ERR_UNSUPPORTED)`` above): the forward
    factors H once (``qpb.factor_box``) and solves with
    ``qpb.solve_box_factored``, whose x may differ from the default's by
    rounding; the backward is ``qpb.solve_box_shared_backward`` on the saved H,
    unchanged.  The default is today's call, bit for bit."""
    if prefactor:
        if H.dim() != 2:
            raise ValueError("prefactor=True needs a 2-D H (n, n): one matrix for the batch")
    return BoxQPFunction.apply(H, f, lb, ub, int(max_iter), float(feas_tol), bool(prefactor))


def solve(H, f, A=None, b=None, meq: int = 0, *, max_iter: int = 0, feas_tol: float = 0.0, prefactor: bool = False):
    """Differentiable batched solve: returns ``(x, status)``; ``x`` carries
    gradients to whichever of H, f, A and b require them, ``status`` (int32 per
    QP) is not differentiable.  QPs whose status is not OK contribute zero
    gradients.  The gradient is the derivative at fixed active set (qpb.h).
    The forward solves every shape ``qpb.solve_eq`` does; the backward needs
    n <= 32 and m <= 64.  H (n, n) and / or A (m, n) may be 2-D: one matrix
    shared by the batch (n <= 32, m <= 64), whose gradient is the sum over the
    batch, computed without a per-QP copy.  ``prefactor=True`` needs a 2-D H
    and (when there are rows) a 2-D A, else ValueError: the forward factors
    them once (``qpb.factor_shared``) and solves with ``qpb.solve_factored``,
    whose x may differ from the default's by rounding; the backward factors
    them once as well (``qpb.factor_shared_backward``,
    ``qpb.solve_factored_backward``), with the default's gradients bit for bit.
    The default is today's call, bit for bit."""
    if prefactor:
        if H.dim() != 2 or (A is not None and A.dim() != 2):
            raise ValueError("prefactor=True needs a 2-D H (n, n) and, with rows, a 2-D A (m, n): one matrix for the batch")
    return QPFunction.apply(H, f, A, b, int(meq), int(max_iter), float(feas_tol), bool(prefactor))
