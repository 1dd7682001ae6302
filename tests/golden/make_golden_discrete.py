#!/usr/bin/env python3
"""Golden EXACT GRADIENTS of the Euler solve, produced by the REFERENCE classes.

Runs only where the reference checkout is present (import shims of make_golden.py).  Executed from the reference,
unchanged: ``ODEBlock.forward`` / ``ODEfunc.forward`` of ode_nn_ngraph_sim.py and ode_nn_ngraphs.py, ``get_sir_t_nodes_torch``
and the loss expressions (ode_nn_ngraph_sim.py:230-234, ode_nn_ngraphs.py:199-203 / :219), then ``loss.backward()`` with
``x.requires_grad_(True)``.  The callable behind ``odeint`` is a plain differentiable Euler loop, y_k = y_{k-1} + (t_k -
t_{k-1}) func(t_{k-1}, y_{k-1}), so torch autograd backpropagates through the solver itself: the gradient of the loss the
forward computes (include/gnode.h gnode_backward_discrete_f32), not torchdiffeq's adjoint rule.

  discrete_karate_B2_H64_T20        karate club, B = 2, H = 64, maxTime 20 (the one-workgroup forward's shape)
  discrete_loops40_B3_H8_T5         40-node graph with self-loops, B = 3, H = 8, maxTime 5
  discrete_er200_B2_H48_T6          Erdos-Renyi G(200, 700), B = 2, H = 48 (the five-launch path), maxTime 6
  discrete_er200_B2_H128_T4         the same graph at H = 128, maxTime 4
  discrete_fbsocial_B1_H64_T30      real fb-social (hub rows), B = 1, H = 64, maxTime 30, deltaT 0.5: 59 intervals
  discrete_multi8_H8_T20            eight real graphs (composition 1-0-2-1-0-3-0-1: 6 844 nodes, hub rows in fb-food,
                                    fb-social and openflights) through ode_nn_ngraphs, H = 8, maxTime 20, graph marker in
                                    column 5

Inputs are those of the input_grad_* fixtures (the same seeds, make_golden_input_grad.py), except that the multi-graph batch
leaves out wiki-vote so that its file stays small.  Each file stores the inputs by seed, "G:<key>" the 8 parameter gradients
and "G:x" x.grad[..., :5] as [rows, 5] of the float64 run, "G32:<key>" / "G32:x" the same classes under torch.float32 (how far
fp32 itself lands from float64: the yardstick; stored as float32, which holds them exactly), "rest_max": max |x.grad[..., 5:]|
of the float64 run, and both losses.
"""
import os
import sys

import networkx as nx
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "gn-ode-sir_amd", "gnode"))
import make_golden as MG  # noqa: E402
import synth  # noqa: E402
from labels import closed_form_labels  # noqa: E402
from make_golden_fullsize import ref_loss, set_params  # noqa: E402
from make_golden_realgraphs import create_graphs, multi_loss  # noqa: E402

KEYS = ["odefunc.linear.weight", "odefunc.linear.bias", "linearS1.weight", "linearS1.bias",
        "linear3.weight", "linear3.bias", "linearS2.weight", "linearS2.bias"]
SYNTH = [("karate", 2, 64, 20, 51), ("loops40", 3, 8, 5, 52), ("er200", 2, 48, 6, 53), ("er200", 2, 128, 4, 54)]


def _euler_odeint(func, y0, t, method="euler", **kw):
    """a plain Euler loop that autograd differentiates through (torchdiffeq's odeint with method='euler' on this grid)"""
    assert method == "euler"
    sol = [y0]
    for k in range(t.shape[0] - 1):
        sol.append(sol[-1] + (t[k + 1] - t[k]) * func(t[k], sol[-1]))
    return torch.stack(sol)


def _use(*modules):
    sys.modules["torchdiffeq"].odeint_adjoint = _euler_odeint
    sys.modules["torchdiffeq"].odeint = _euler_odeint
    for m in modules:
        m.odeint = _euler_odeint


def _run(make_model, x, P, loss_fn):
    """float64 and float32 runs -> dict of G:*, G32:*, rest_max, loss, loss32"""
    d = {}
    for dtype, pre in [(torch.float64, "G:"), (torch.float32, "G32:")]:
        torch.set_default_dtype(dtype)
        mdl = make_model()
        set_params(mdl, P, dtype)
        xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
        S, I, R = mdl(xt)
        loss = loss_fn(S, I, R)
        loss.backward()
        sd = dict(mdl.named_parameters())
        for k in KEYS:
            d[pre + k] = sd[k].grad.detach().numpy().copy()
        g = xt.grad.detach().numpy().reshape(-1, x.shape[-1])
        d[pre + "x"] = g[:, :5].copy()
        d["loss" + ("" if dtype == torch.float64 else "32")] = np.float64(loss.item())
        if dtype == torch.float64:
            d["rest_max"] = np.float64(np.abs(g[:, 5:]).max())
    torch.set_default_dtype(torch.float32)
    return d


def _yard(d):
    """max |G32 - G| / max |G| per gradient"""
    return {k: float(np.abs(d["G32:" + k] - d["G:" + k]).max() / np.abs(d["G:" + k]).max()) for k in KEYS + ["x"]}


def main():
    MG._install_import_shims()
    _use()
    sys.path.insert(0, MG.REF)
    cwd = os.getcwd()
    os.chdir("/tmp")
    import ode_nn_ngraph_sim as single
    import ode_nn_ngraphs as multi
    import ode_nn as helpers
    os.chdir(cwd)
    _use(single, multi)
    dev = torch.device("cpu")
    graphs = MG._graphs()
    for gname, B, H, maxTime, seed in SYNTH:
        G = graphs[gname]
        A = nx.adjacency_matrix(G)
        n, deltaT = A.shape[0], 0.5
        P = synth.linear_params(H, seed=seed)
        x = synth.samples(n, B, H, seed=seed + 100)
        y = torch.from_numpy(closed_form_labels(B, n, maxTime)).to(torch.float64)
        make = lambda: single.ODEBlock(maxTime, deltaT, n, [0], H, single.ODEfunc(A, 0.2, 0.1, H, dev), dev)
        d = _run(make, x, P, lambda S, I, R: ref_loss(helpers, S, I, R, y, maxTime, deltaT))
        d.update(n=np.int32(n), B=np.int32(B), H=np.int32(H), maxTime=np.int32(maxTime), deltaT=np.float64(deltaT),
                 param_seed=np.int32(seed), sample_seed=np.int32(seed + 100), method=np.asarray("euler"),
                 edges=np.asarray(list(G.edges()), dtype=np.int32))
        tag = f"discrete_{gname}_B{B}_H{H}_T{maxTime}"
        np.savez_compressed(os.path.join(HERE, tag + ".npz"), **d)
        print("wrote", tag, "loss", d["loss"], "rest", d["rest_max"], "fp32 yardstick", _yard(d))

    A_list = create_graphs()
    ns = [a.shape[0] for a in A_list]
    import fixture_cases as FC
    gs = FC.graphs()
    # fb-social: the inputs of input_grad_fbsocial_B1_H64_T30
    H, maxTime, deltaT = 64, 30, 0.5
    d0 = dict(graph=np.int32(2), B=np.int32(1), H=np.int32(H), maxTime=np.int32(maxTime), deltaT=np.float64(deltaT),
              param_seed=np.int32(61), sample_seed=np.int32(6100), beta_scale=np.float64(0.1), method=np.asarray("euler"))
    x, P, y = FC.inputs(d0, gs)
    A, n = A_list[2], ns[2]
    make = lambda: single.ODEBlock(maxTime, deltaT, n, [0], H, single.ODEfunc(A, 0.2, 0.1, H, dev), dev)
    yt = torch.from_numpy(y.reshape(1, n, maxTime, 3)).to(torch.float64)
    d = _run(make, x, P, lambda S, I, R: ref_loss(helpers, S, I, R, yt, maxTime, deltaT))
    d.update(d0)
    np.savez_compressed(os.path.join(HERE, "discrete_fbsocial_B1_H64_T30.npz"), **d)
    print("wrote fbsocial loss", d["loss"], "rest", d["rest_max"], "fp32 yardstick", _yard(d))
    # eight real graphs at H = 8: the seeds of input_grad_multi8_H8_T20, a composition without wiki-vote
    H, maxTime = 8, 20
    d0 = dict(picks=np.asarray([1, 0, 2, 1, 0, 3, 0, 1], dtype=np.int32), H=np.int32(H), maxTime=np.int32(maxTime),
              deltaT=np.float64(deltaT), param_seed=np.int32(62), sample_seed=np.int32(6200), beta_scale=np.float64(0.03),
              method=np.asarray("euler"))
    x, P, y = FC.inputs(d0, gs)
    make = lambda: multi.ODEBlock(maxTime, deltaT, H, multi.ODEfunc(A_list, H, dev), dev)
    yt = torch.from_numpy(y).to(torch.float64)
    d = _run(make, x, P, lambda S, I, R: multi_loss(helpers, S, I, R, yt, maxTime, deltaT))
    d.update(d0)
    np.savez_compressed(os.path.join(HERE, "discrete_multi8_H8_T20.npz"), **d)
    print("wrote multi8 loss", d["loss"], "rest", d["rest_max"], "fp32 yardstick", _yard(d))


if __name__ == "__main__":
    main()
