#!/usr/bin/env python3
"""Golden PARAMETER GRADIENTS of ODEBlock under the RK4 (3/8 rule) adjoint, produced by the REFERENCE classes.

Runs only where the reference checkout is (the helpers and import shims of make_golden_adjoint.py / make_golden.py).
Executed from the reference, unchanged: ``ODEBlock.forward`` (encoder, the ``odeint`` call, read-out head, softmax),
``ODEfunc.forward`` -- every vector-Jacobian product below is torch autograd through it --, ``get_sir_t_nodes_torch``
and the loss expression of ode_nn_ngraph_sim.py:230-234, then ``loss.backward()``.

The reference hard-codes ``method='euler'`` in its odeint call (ode_nn_ngraph_sim.py:168); the callable installed as its
``odeint`` here (_AdjointRK4) IGNORES that string and restates torchdiffeq 0.2.2's ``odeint_adjoint(..., method='rk4')``:
forward = the 3/8-rule step on every grid interval under no_grad; backward = per interval i = G-1 .. 1 one 3/8-rule step of
size h = -dt of the augmented system (f(y), -a^T df/dy, -a^T df/dtheta) from t_i to t_{i-1}, y reset to the stored
sol[i-1] and the output cotangent of grid point i-1 added.  torchdiffeq itself is absent, so the rule is parity-unpinned
(DESIGN.md section 7), as the Euler rule is.

  rk4_adjoint_karate_H64_T20.npz   karate club, B = 2, H = 64, maxTime = 20, deltaT = 0.5 (39 intervals)
  rk4_adjoint_loops40_H8_T5.npz    the 40-node graph with self-loops, B = 3, H = 8, maxTime = 5
Each: the seeds of the parameters and samples (gnode/synth.py), the edge list, the loss, the 8 gradients in float64
("G:<name>") and the same classes and rule run under torch.float32 ("G32:<name>": the yardstick of what fp32 reaches).
"""
import os
import sys

import numpy as np
import networkx as nx
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "gn-ode-sir_amd", "gnode"))
import make_golden as MG  # noqa: E402
import synth  # noqa: E402
from labels import closed_form_labels  # noqa: E402
from make_golden_fullsize import ref_loss, set_params  # noqa: E402


def _rk4(F, y, h):
    """torchdiffeq 0.2.2 rk4_alt_step_func on a tuple state: the increment of one step of size h."""
    third = 1.0 / 3.0
    k1 = F(y)
    k2 = F(tuple(a + h * b * third for a, b in zip(y, k1)))
    k3 = F(tuple(a + h * (c - b * third) for a, b, c in zip(y, k1, k2)))
    k4 = F(tuple(a + h * (b - c + d) for a, b, c, d in zip(y, k1, k2, k3)))
    return tuple((b + 3 * (c + d) + e) * h * 0.125 for b, c, d, e in zip(k1, k2, k3, k4))


class _AdjointRK4(torch.autograd.Function):
    """torchdiffeq's OdeintAdjointMethod under fixed-grid rk4, restated (see the module docstring)."""

    @staticmethod
    def forward(ctx, func, t, n_params, y0, *params):
        with torch.no_grad():
            sol = [y0]
            for k in range(t.shape[0] - 1):
                sol.append(sol[-1] + _rk4(lambda s: (func(t[k], s[0]),), (sol[-1],), t[k + 1] - t[k])[0])
            sol = torch.stack(sol)
        ctx.func, ctx.t, ctx.params = func, t, params
        ctx.save_for_backward(sol)
        return sol

    @staticmethod
    def backward(ctx, gsol):
        (sol,) = ctx.saved_tensors
        func, t, params = ctx.func, ctx.t, ctx.params

        def aug(s):
            # the augmented dynamics of torchdiffeq: (f, -a^T df/dy, -a^T df/dtheta), VJPs by autograd through the
            # reference's ODEfunc
            y, a = s[0], s[1]
            with torch.enable_grad():
                yy = y.detach().requires_grad_(True)
                f = func(t[0], yy)
                vj = torch.autograd.grad(f, (yy,) + tuple(params), -a, allow_unused=True)
            return (f.detach(), vj[0]) + tuple(torch.zeros_like(p) if v is None else v for p, v in zip(params, vj[1:]))

        a = gsol[-1].clone()
        gp = [torch.zeros_like(p) for p in params]
        for i in range(sol.shape[0] - 1, 0, -1):
            h = t[i - 1] - t[i]
            inc = _rk4(aug, (sol[i], a, *[torch.zeros_like(p) for p in params]), h)
            a = a + inc[1] + gsol[i - 1]
            for g, v in zip(gp, inc[2:]):
                g += v
        return (None, None, None, a, *gp)


def _odeint_adjoint(func, y0, t, method="euler", **kw):
    # method: the reference passes 'euler' (ode_nn_ngraph_sim.py:168); this shim runs rk4 regardless
    params = tuple(p for p in func.parameters() if p.requires_grad)
    return _AdjointRK4.apply(func, t, len(params), y0, *params)


def main():
    MG._install_import_shims()
    sys.modules["torchdiffeq"].odeint_adjoint = _odeint_adjoint
    sys.modules["torchdiffeq"].odeint = _odeint_adjoint
    sys.path.insert(0, MG.REF)
    cwd = os.getcwd()
    os.chdir("/tmp")
    import ode_nn_ngraph_sim as single
    import ode_nn as helpers
    os.chdir(cwd)
    dev = torch.device("cpu")
    graphs = MG._graphs()
    keys = ["odefunc.linear.weight", "odefunc.linear.bias", "linearS1.weight", "linearS1.bias",
            "linear3.weight", "linear3.bias", "linearS2.weight", "linearS2.bias"]
    for gname, B, H, maxTime in [("karate", 2, 64, 20), ("loops40", 3, 8, 5)]:
        G = graphs[gname]
        A = nx.adjacency_matrix(G)
        n, deltaT = A.shape[0], 0.5
        seed = {"karate": 41, "loops40": 43}[gname]
        P = synth.linear_params(H, seed=seed)
        x = synth.samples(n, B, H, seed=seed + 100)
        d = dict(n=np.int32(n), B=np.int32(B), H=np.int32(H), maxTime=np.int32(maxTime), deltaT=np.float64(deltaT),
                 param_seed=np.int32(seed), sample_seed=np.int32(seed + 100), edges=np.asarray(list(G.edges()), dtype=np.int32))
        for dtype, pre in [(torch.float64, "G:"), (torch.float32, "G32:")]:
            torch.set_default_dtype(dtype)
            f = single.ODEfunc(A, 0.2, 0.1, H, dev)
            mdl = single.ODEBlock(maxTime, deltaT, n, [0], H, f, dev)
            set_params(mdl, P, dtype)
            y = torch.from_numpy(closed_form_labels(B, n, maxTime)).to(torch.float64)
            mdl.zero_grad()
            S, I, R = mdl(torch.from_numpy(x).to(dtype))
            loss = ref_loss(helpers, S, I, R, y, maxTime, deltaT)
            loss.backward()
            named = dict(mdl.named_parameters())
            for k in keys:
                d[pre + k] = named[k].grad.detach().numpy().astype(np.float64)
            d["loss" if dtype == torch.float64 else "loss32"] = np.float64(loss.item())
        torch.set_default_dtype(torch.float32)
        tag = f"rk4_adjoint_{gname}_H{H}_T{maxTime}"
        np.savez_compressed(os.path.join(HERE, tag + ".npz"), **d)
        rel = {k: float(np.abs(d["G32:" + k] - d["G:" + k]).max() / max(np.abs(d["G:" + k]).max(), 1e-30)) for k in keys}
        print("wrote", tag, "loss", d["loss"], "fp32 vs float64:", {k: f"{v:.1e}" for k, v in rel.items()})


if __name__ == "__main__":
    main()
