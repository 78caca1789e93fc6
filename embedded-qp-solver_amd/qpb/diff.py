"""qpb.diff -- the solver as a differentiable torch function.

``solve(H, f, A, b, meq)`` is ``qpb.solve_eq`` with gradients: the backward
pass is ``qpb.solve_backward`` (qpb_solve_backward, one KKT solve per QP at the
solution's active set, on the GPU).  This module imports torch at the top;
``import qpb`` itself stays torch-free.

    x, status = qpb.diff.solve(H, f, A, b, meq=2)   # H, f, A, b may require grad
    loss = (w * x).sum()
    loss.backward()                                 # H.grad, f.grad, A.grad, b.grad
"""
from __future__ import annotations

import torch

import qpb


class QPFunction(torch.autograd.Function):
    """x*(H, f, A, b) of min 1/2 x'Hx + f'x s.t. A[:meq] x = b[:meq], A[meq:] x <= b[meq:]."""

    @staticmethod
    def forward(ctx, H, f, A, b, meq, max_iter, feas_tol):
        H, f = H.contiguous(), f.contiguous()
        if A is not None:
            A, b = A.contiguous(), b.contiguous()
        sol = qpb.solve_eq(H, f, A, b, meq, max_iter=max_iter, feas_tol=feas_tol) if A is not None \
            else qpb.solve(H, f, max_iter=max_iter, feas_tol=feas_tol)
        ctx.has_rows = A is not None
        ctx.save_for_backward(H, A, sol.x, sol.lam, sol.active, sol.status)
        ctx.mark_non_differentiable(sol.status)
        return sol.x, sol.status

    @staticmethod
    def backward(ctx, gx, _gstatus):
        H, A, x, lam, active, status = ctx.saved_tensors
        wanted = [k for k, w in zip("HfAb", ctx.needs_input_grad[:4]) if w and (ctx.has_rows or k in "Hf")]
        if not wanted:
            return (None,) * 7
        sol = qpb.Solution(x, lam, active, status, None)
        # on torch's current stream; above n = 32 or m = 64 this raises QPBError(ERR_UNSUPPORTED)
        gH, gf, gA, gb = qpb.solve_backward(H, A, sol, gx.contiguous(), need=wanted)
        return gH, gf, gA, gb, None, None, None


def solve(H, f, A=None, b=None, meq: int = 0, *, max_iter: int = 0, feas_tol: float = 0.0):
    """Differentiable batched solve: returns ``(x, status)``; ``x`` carries
    gradients to whichever of H, f, A and b require them, ``status`` (int32 per
    QP) is not differentiable.  QPs whose status is not OK contribute zero
    gradients.  The gradient is the derivative at fixed active set (qpb.h).
    The forward solves every shape ``qpb.solve_eq`` does; the backward needs
    n <= 32 and m <= 64."""
    return QPFunction.apply(H, f, A, b, int(meq), int(max_iter), float(feas_tol))
