"""Autograd bridge for ODEBlock.forward.

Inference (no_grad, or nothing requires grad) calls the fused forward and never
materialises the trajectory.  Training saves `sol` as torchdiffeq's
odeint_adjoint does and runs its adjoint backward in libgnode_hip.so: the
adjoint-Euler sweep (method='euler') or the RK4 (3/8 rule)
adjoint (method='rk4'), or with adjoint=False the exact gradient
of the Euler solve.  `rhs` is ODEfunc.forward as an
autograd node over the RHS and its vector-Jacobian product.
"""
from __future__ import annotations

import torch

from . import ops


def _needs_grad(params: dict, x2d=None) -> bool:
    return torch.is_grad_enabled() and (any(p.requires_grad for p in params.values()) or
                                        (x2d is not None and x2d.requires_grad))


class _GNODEForward(torch.autograd.Function):
    @staticmethod
    def forward(ctx, graph, x2d, dts, method, out_rows, adjoint, keys, *tensors):
        params = dict(zip(keys, tensors))
        # an input gradient needs the recomputing backward: no kept activations, the trajectory carries A Z_I instead.  The
        # exact (adjoint=False) gradient runs over the kept activations like the adjoint (backward passes ctx.keep explicitly),
        # except where its plan stays recomputing whatever is kept (one-workgroup-size graphs, 2-point grids)
        want_keep = False if ctx.needs_input_grad[1] else None
        if want_keep is None and not adjoint and x2d.shape[1] - 3 == 64 and \
                ops.discrete_path(graph, x2d.shape[0], 64, len(dts), out_rows, keep=True) == 0:
            want_keep = False
        S, I, R, sol = ops.forward(graph, x2d.detach(), params, dts, method, out_rows, want_sol=True, want_keep=want_keep)
        ctx.graph, ctx.dts, ctx.method, ctx.out_rows, ctx.adjoint, ctx.keys = graph, dts, method, out_rows, adjoint, keys
        ctx.keep = sol.gnode_keep            # kept activations (a plain buffer nothing else references), or None
        ctx.save_for_backward(x2d, sol, *tensors)
        return S, I, R

    @staticmethod
    def backward(ctx, gS, gI, gR):
        x2d, sol, *tensors = ctx.saved_tensors
        params = dict(zip(ctx.keys, tensors))
        ref = next(g for g in (gS, gI, gR) if g is not None)          # an output the loss did not use has no gradient
        gS, gI, gR = (torch.zeros_like(ref) if g is None else g for g in (gS, gI, gR))
        want_x = ctx.needs_input_grad[1]
        want_params = any(ctx.needs_input_grad[7:])
        grads = ops.backward(ctx.graph, x2d.detach(), params, ctx.dts, ctx.method, ctx.out_rows, sol,
                             gS.contiguous(), gI.contiguous(), gR.contiguous(), keep=ctx.keep, want_x=want_x,
                             want_params=want_params, adjoint=ctx.adjoint)
        # (ctx.keep stays: a second backward through this node -- retain_graph=True, two losses on one forward --
        #  needs it again; it is freed with ctx and sol)
        gx = grads["x"].to(x2d.dtype) if want_x else None
        return (None, gx, None, None, None, None, None,
                *[grads[k] if need else None for k, need in zip(ctx.keys, ctx.needs_input_grad[7:])])


def forward_with_grad(graph, x2d, params, dts, method="euler", out_rows=None, adjoint=True):
    """adjoint=False: the backward is the exact gradient of the Euler solve (ops.backward(adjoint=False)); it raises for rk4."""
    adjoint = ops._check_adjoint(adjoint, method)
    if not _needs_grad(params, x2d):
        with torch.no_grad():
            S, I, R, _ = ops.forward(graph, x2d, {k: v.detach() for k, v in params.items()}, dts, method, out_rows)
        return S, I, R
    keys = tuple(params.keys())
    return _GNODEForward.apply(graph, x2d, dts, method, out_rows, adjoint, keys, *[params[k] for k in keys])


class _RHSFunction(torch.autograd.Function):
    """ODEfunc.forward (ode_nn_ngraph_sim.py:58-96) as an autograd node: the value from `ops.rhs`, the backward from ONE
    `ops.rhs_vjp` pass -- what torchdiffeq's odeint_adjoint asks of the reference's ODEfunc (torch.autograd.grad of
    func(t, y) with respect to y and the parameters)."""

    @staticmethod
    def forward(ctx, graph, x, W, b):
        ctx.graph = graph
        ctx.save_for_backward(x, W, b)
        return ops.rhs(graph, x, W, b)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, W, b = ctx.saved_tensors
        _, want_x, want_W, want_b = ctx.needs_input_grad
        if not (want_x or want_W or want_b):
            return None, None, None, None
        _, dx, dW, db = ops.rhs_vjp(ctx.graph, x, W.detach(), b.detach(), g.contiguous(), want_f=False,
                                    want_y=want_x, want_W=want_W, want_b=want_b)
        return None, dx, dW, db


def rhs(graph, x, W, b):
    """Differentiable RHS: x [4*rows, H] -> dx; gradients flow to x, W and b as they require it."""
    return _RHSFunction.apply(graph, x, W, b)


class _L1LossSum(torch.autograd.Function):
    """sum |cat(S, I, R)[rows, T, 3][:, t0:, :] - y[:, t0:, :]| with its gradient from one kernel (csrc/gnode_loss.hip)."""

    @staticmethod
    def forward(ctx, S, I, R, y, t0):
        need_grad = any(ctx.needs_input_grad[:3])
        total, sgn = ops.l1_loss_sum(S, I, R, y, t0, want_sign=need_grad)
        ctx.shape = S.shape
        if need_grad:
            ctx.save_for_backward(sgn)
        return total

    @staticmethod
    def backward(ctx, g):
        (sgn,) = ctx.saved_tensors
        gs = (sgn * g.to(torch.float32)).view(3, *ctx.shape)
        return gs[0], gs[1], gs[2], None, None


def l1_loss_sum(S, I, R, y, t0=1):
    """The reference's loss numerator (ode_nn_ngraph_sim.py:230-234): S, I, R are the model's [T, rows(, 1)] outputs,
    y the labels [rows, T, 3] (fp32 or fp64); returns a float64 scalar.  Divide by rows * (T - t0) * 3 for L1Loss's mean."""
    return _L1LossSum.apply(S, I, R, y, t0)


def l1_loss_mean_backward(S, I, R, y, count, t0=1):
    """loss.backward() for  loss = l1_loss_sum(S, I, R, y, t0) / count  (the trainer's step, ode_nn_ngraph_sim.py:234-236) without
    the scalar graph in between: the loss kernel writes sign(pred - y) / count, which IS dloss/d(S, I, R), and the backward
    of the model starts from it -- five tiny launches less per step (division, ones, division's backward, a cast, a multiply).
    Returns the loss SUM (float64 device scalar), as l1_loss_sum does.  Bit-identical gradients: the scalar path multiplies
    the signs by the same fp32(1 / count)."""
    total, sgn = ops.l1_loss_sum(S, I, R, y, t0, want_sign=True, sign_scale=1.0 / float(count))
    gs = sgn.view(3, *S.shape)
    torch.autograd.backward([S, I, R], [gs[0], gs[1], gs[2]])
    return total
