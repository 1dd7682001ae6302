"""float64 restatement of the ODEBlock input gradient dL/dx (include/gnode.h gnode_backward_dx_f32),
written from the spec's formulas: the adjoint sweep of torchdiffeq 0.2.2's odeint_adjoint (Euler, or the RK4 3/8 rule) with
the RHS vector-Jacobian product of rhs_vjp_restate.rhs_vjp -- whose beta-gamma slab is
    d/dbeta = sum_h (a_I - a_S) AI Z_S        d/dgamma = sum_h (a_R - a_I) Z_I        (AI = A Z_I, at y_i / the stage state)
and which feeds nothing back into a_S, a_I, a_R --, then the encoder
    dL/dX0 = sum_h a_X(t0) [sol0_X > 0] linearS1.weight[h]        (X = S, I, R)
and the remaining columns of the slab 0.  The fixtures it is held to (tests/golden/input_grad_*.npz) are autograd through
the reference's own classes, so agreement pins these formulas to the reference."""
from __future__ import annotations

import numpy as np
import torch

from rhs_vjp_restate import _index, l1_loss_of, rhs, rhs_vjp, rk4_step


def input_grad(x2d, P, rowptr, col, n, maxTime, deltaT, y_labels, method="euler"):
    """dL/dx2d [rows, 3+H] (numpy float64) for the reference's L1 loss (ode_nn_ngraph_sim.py:230-234) against y_labels
    [rows, T, 3] at the integer times.  x2d [rows, 3+H]; rows a multiple of n (graph `rowptr`, `col` per sample)."""
    dt64 = torch.float64
    t = lambda a: torch.tensor(np.asarray(a), dtype=dt64)
    Pt = {k: t(v) for k, v in P.items()}
    x2 = t(x2d)
    rows, q = x2.shape[0], x2.shape[0]
    ridx, cidx = _index(rowptr, col, n, rows)
    W, b, w1 = Pt["odefunc.linear.weight"], Pt["odefunc.linear.bias"], Pt["linearS1.weight"][:, 0]
    enc = lambda s: torch.relu(torch.nn.functional.linear(s.unsqueeze(-1), Pt["linearS1.weight"], Pt["linearS1.bias"]))
    y0 = torch.cat((enc(x2[:, 0]), enc(x2[:, 1]), enc(x2[:, 2]), x2[:, 3:]))
    grid = np.arange(0, maxTime, deltaT)
    dts = (grid[1:] - grid[:-1]).astype(np.float32).astype(np.float64)
    f = lambda y: rhs(y, W, b, ridx, cidx)
    sol = [y0]
    for dt in dts:
        sol.append(sol[-1] + (rk4_step(f, sol[-1], float(dt)) if method == "rk4" else float(dt) * f(sol[-1])))
    sol = torch.stack(sol)
    # the head's VJP: ordinary autograd on the trajectory (as the reference's loss.backward() takes it)
    sol_leaf = sol.clone().requires_grad_(True)
    ro = lambda Y: torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(Y, Pt["linear3.weight"], Pt["linear3.bias"])),
                                              Pt["linearS2.weight"], Pt["linearS2.bias"])
    out = torch.softmax(torch.cat((ro(sol_leaf[:, :q]), ro(sol_leaf[:, q:2 * q]), ro(sol_leaf[:, 2 * q:3 * q])), -1), 2)
    out_rows = [int(i / deltaT) for i in range(int(maxTime))]
    L = l1_loss_of(y_labels, out_rows)(out[..., 0], out[..., 1], out[..., 2])
    (gsol,) = torch.autograd.grad(L, [sol_leaf])
    V = lambda y, a: rhs_vjp(y, W, b, a, ridx, cidx)[1]          # a^T df/dy, beta-gamma slab from the formulas above
    a = gsol[-1].clone()
    for i in range(sol.shape[0] - 1, 0, -1):
        dt = float(dts[i - 1])
        if method == "rk4":
            # the 3/8 rule on (y, a) with h = -dt and rates (f, -V): torchdiffeq's augmented dynamics
            h, third = -dt, 1.0 / 3.0
            F = lambda s: (f(s[0]), -V(s[0], s[1]))
            st = (sol[i], a)
            k1 = F(st)
            k2 = F(tuple(s + h * k * third for s, k in zip(st, k1)))
            k3 = F(tuple(s + h * (c2 - c1 * third) for s, c1, c2 in zip(st, k1, k2)))
            k4 = F(tuple(s + h * (c1 - c2 + c3) for s, c1, c2, c3 in zip(st, k1, k2, k3)))
            a = a + (k1[1] + 3 * (k2[1] + k3[1]) + k4[1]) * h * 0.125 + gsol[i - 1]
        else:
            a = a + dt * V(sol[i], a) + gsol[i - 1]
    gx = torch.zeros_like(x2)
    for X in range(3):
        gx[:, X] = (a[X * q:(X + 1) * q] * (sol[0, X * q:(X + 1) * q] > 0) * w1).sum(1)
    gx[:, 3:] = a[3 * q:]
    return gx.numpy()
