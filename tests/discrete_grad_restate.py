"""float64 restatement of the exact gradient of the Euler solve (include/gnode.h gnode_backward_discrete_f32; DESIGN section
7.3): torch autograd through a plain Euler loop y_k = y_{k-1} + dt_{k-1} f(y_{k-1}) of rhs_vjp_restate.rhs, then the head and
the encoder -- exact by construction.  The fixtures it is held to (tests/golden/discrete_*.npz) are autograd through the
reference's own classes under the same loop, so agreement pins the restatement to the reference; the GPU is then held to
both."""
from __future__ import annotations

import numpy as np
import torch

from rhs_vjp_restate import _index, l1_loss_of, rhs

KEYS = ("odefunc.linear.weight", "odefunc.linear.bias", "linearS1.weight", "linearS1.bias",
        "linear3.weight", "linear3.bias", "linearS2.weight", "linearS2.bias")


def discrete_grads(x2d, P, rowptr, col, n, dts, loss_of_outputs, dtype=torch.float64):
    """{8 parameter gradients, "x": dL/dx2d [rows, 3+H]} as float64 numpy for loss_of_outputs(S, I, R) (each [G, rows] torch)
    of the Euler forward on the fp32 step sizes `dts`.  x2d [rows, 3+H]; rows a multiple of n (graph rowptr, col per sample)."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    Pt = {k: t(v).requires_grad_(True) for k, v in P.items()}
    x2 = t(x2d).requires_grad_(True)
    q = x2.shape[0]
    ridx, cidx = _index(rowptr, col, n, q)
    enc = lambda s: torch.relu(torch.nn.functional.linear(s.unsqueeze(-1), Pt["linearS1.weight"], Pt["linearS1.bias"]))
    y = torch.cat((enc(x2[:, 0]), enc(x2[:, 1]), enc(x2[:, 2]), x2[:, 3:]))
    sol = [y]
    for dt in np.asarray(dts, dtype=np.float32).astype(np.float64):
        sol.append(sol[-1] + float(dt) * rhs(sol[-1], Pt["odefunc.linear.weight"], Pt["odefunc.linear.bias"], ridx, cidx))
    sol = torch.stack(sol)
    ro = lambda Y: torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(Y, Pt["linear3.weight"], Pt["linear3.bias"])),
                                              Pt["linearS2.weight"], Pt["linearS2.bias"])
    out = torch.softmax(torch.cat((ro(sol[:, :q]), ro(sol[:, q:2 * q]), ro(sol[:, 2 * q:3 * q])), -1), 2)
    L = loss_of_outputs(out[..., 0], out[..., 1], out[..., 2])
    gr = torch.autograd.grad(L, [Pt[k] for k in KEYS] + [x2])
    res = {k: g.detach().numpy().astype(np.float64) for k, g in zip(KEYS, gr[:-1])}
    res["x"] = gr[-1].detach().numpy().astype(np.float64)
    return res


def reference_loss_grads(x2d, P, rowptr, col, n, maxTime, deltaT, y_labels):
    """discrete_grads for the reference's L1 loss (ode_nn_ngraph_sim.py:230-234) against y_labels [rows, T, 3] at the
    integer times (get_sir_t_nodes_torch)."""
    grid = np.arange(0, maxTime, deltaT)
    dts = (grid[1:] - grid[:-1]).astype(np.float32)
    out_rows = [int(i / deltaT) for i in range(int(maxTime))]
    return discrete_grads(x2d, P, rowptr, col, n, dts, l1_loss_of(y_labels, out_rows))


def linear_loss(gS, gI, gR, out_rows=None):
    """sum(gS * S[out_rows]) + ...: the loss whose upstream gradients are gS, gI, gR ([n_out, rows] numpy)"""
    g = [torch.from_numpy(np.asarray(a, dtype=np.float64)) for a in (gS, gI, gR)]
    idx = None if out_rows is None else torch.as_tensor(np.asarray(out_rows), dtype=torch.int64)

    def L(S, I, R):
        pick = (lambda A: A) if idx is None else (lambda A: A[idx])
        return sum((pick(A) * gA.to(A.dtype)).sum() for A, gA in zip((S, I, R), g))
    return L
