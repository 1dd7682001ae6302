#!/usr/bin/env python3
"""Golden INPUT GRADIENTS x.grad of ODEBlock, produced by the REFERENCE classes.

Runs only where the reference checkout is present (import shims of make_golden.py).  Executed from the reference,
unchanged: ``ODEBlock.forward`` / ``ODEfunc.forward`` of ode_nn_ngraph_sim.py and ode_nn_ngraphs.py, ``get_sir_t_nodes_torch``
and the loss expressions (ode_nn_ngraph_sim.py:230-234, ode_nn_ngraphs.py:199-203 / :219), then ``loss.backward()`` with
``x.requires_grad_(True)``.  The callable behind ``odeint`` is this repo's restatement of torchdiffeq 0.2.2's adjoint
(make_golden_adjoint._odeint_adjoint: Euler; make_golden_rk4_adjoint._odeint_adjoint: the 3/8 rule), whose backward
returns the adjoint at t0 for the WHOLE state, beta-gamma slab included -- what odeint_adjoint hands to x.

  input_grad_karate_B2_H64_T20        karate club, B = 2, H = 64, maxTime 20 (the one-workgroup forward's shape)
  input_grad_loops40_B3_H8_T5         40-node graph with self-loops, B = 3, H = 8, maxTime 5
  input_grad_er200_B2_H48_T6          Erdos-Renyi G(200, 700), B = 2, H = 48 (the five-launch path), maxTime 6
  input_grad_er200_B2_H128_T4         the same graph at H = 128, maxTime 4
  input_grad_fbsocial_B1_H64_T30      real fb-social (hub rows), B = 1, H = 64, maxTime 30, deltaT 0.5: 59 intervals
  input_grad_multi8_H8_T20            eight real graphs (composition 4-2-3-1-0-4-2-3) through ode_nn_ngraphs, H = 8,
                                      maxTime 20, graph marker in column 5
  input_grad_rk4_karate_B2_H64_T20    karate club under the RK4 (3/8 rule) adjoint, B = 2, H = 64

Each stores the inputs by seed (gnode/synth.py; real graphs by index into real_graphs.npz, the multi-graph batch as
fixture_cases.inputs rebuilds it), "GX": x.grad[..., :5] as [rows, 5] of the float64 run, "yard32": how far the same
classes and rule run under float32 land from it -- max |GX32 - GX| / max |GX| over columns {S0, I0, R0} and over {beta,
gamma}: the yardstick --, "rest_max": max |x.grad[..., 5:]| of the float64 run, and both losses.
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
import make_golden_adjoint as ADJ  # noqa: E402
import make_golden_rk4_adjoint as ADJ4  # noqa: E402
import synth  # noqa: E402
from labels import closed_form_labels  # noqa: E402
from make_golden_fullsize import ref_loss, set_params  # noqa: E402
from make_golden_realgraphs import create_graphs, multi_loss  # noqa: E402

SYNTH = [("karate", 2, 64, 20, 51, "euler"), ("loops40", 3, 8, 5, 52, "euler"), ("er200", 2, 48, 6, 53, "euler"),
         ("er200", 2, 128, 4, 54, "euler"), ("karate", 2, 64, 20, 55, "rk4")]


def _use(method, *modules):
    """install the restated adjoint of `method` as torchdiffeq's and as the name the reference modules imported"""
    f = ADJ._odeint_adjoint if method == "euler" else ADJ4._odeint_adjoint
    sys.modules["torchdiffeq"].odeint_adjoint = f
    sys.modules["torchdiffeq"].odeint = f
    for m in modules:
        m.odeint = f


def _run(make_model, x, P, loss_fn):
    """float64 and float32 runs -> dict (GX, yard32, rest_max, loss, loss32)"""
    d = {}
    for dtype, pre in [(torch.float64, ""), (torch.float32, "32")]:
        torch.set_default_dtype(dtype)
        mdl = make_model()
        set_params(mdl, P, dtype)
        xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
        S, I, R = mdl(xt)
        loss = loss_fn(S, I, R)
        loss.backward()
        g = xt.grad.detach().numpy().astype(np.float64).reshape(-1, x.shape[-1])
        d["GX" + pre] = g[:, :5]
        d["loss" + pre] = np.float64(loss.item())
        if dtype == torch.float64:
            d["rest_max"] = np.float64(np.abs(g[:, 5:]).max())
    torch.set_default_dtype(torch.float32)
    g32 = d.pop("GX32")
    d["yard32"] = np.asarray([np.abs(g32[:, c] - d["GX"][:, c]).max() / np.abs(d["GX"][:, c]).max()
                              for c in (slice(0, 3), slice(3, 5))], dtype=np.float64)
    return d


def _yard(d):
    return dict(zip(("SIR0", "bg"), d["yard32"].tolist()))


def main():
    MG._install_import_shims()
    _use("euler")
    sys.path.insert(0, MG.REF)
    cwd = os.getcwd()
    os.chdir("/tmp")
    import ode_nn_ngraph_sim as single
    import ode_nn_ngraphs as multi
    import ode_nn as helpers
    os.chdir(cwd)
    dev = torch.device("cpu")
    graphs = MG._graphs()
    for gname, B, H, maxTime, seed, method in SYNTH:
        _use(method, single)
        G = graphs[gname]
        A = nx.adjacency_matrix(G)
        n, deltaT = A.shape[0], 0.5
        P = synth.linear_params(H, seed=seed)
        x = synth.samples(n, B, H, seed=seed + 100)
        y = torch.from_numpy(closed_form_labels(B, n, maxTime)).to(torch.float64)
        make = lambda: single.ODEBlock(maxTime, deltaT, n, [0], H, single.ODEfunc(A, 0.2, 0.1, H, dev), dev)
        d = _run(make, x, P, lambda S, I, R: ref_loss(helpers, S, I, R, y, maxTime, deltaT))
        d.update(n=np.int32(n), B=np.int32(B), H=np.int32(H), maxTime=np.int32(maxTime), deltaT=np.float64(deltaT),
                 param_seed=np.int32(seed), sample_seed=np.int32(seed + 100), method=np.asarray(method),
                 edges=np.asarray(list(G.edges()), dtype=np.int32))
        tag = f"input_grad_{'rk4_' if method == 'rk4' else ''}{gname}_B{B}_H{H}_T{maxTime}"
        np.savez_compressed(os.path.join(HERE, tag + ".npz"), **d)
        print("wrote", tag, "loss", d["loss"], "rest", d["rest_max"], "fp32 yardstick", _yard(d))

    _use("euler", single, multi)
    A_list = create_graphs()
    ns = [a.shape[0] for a in A_list]
    import fixture_cases as FC
    gs = FC.graphs()
    # fb-social, configs[1]'s shape, the seeds and beta scale of real_single_fbsocial_H64_T30
    H, maxTime, deltaT = 64, 30, 0.5
    d0 = dict(graph=np.int32(2), B=np.int32(1), H=np.int32(H), maxTime=np.int32(maxTime), deltaT=np.float64(deltaT),
              param_seed=np.int32(61), sample_seed=np.int32(6100), beta_scale=np.float64(0.1), method=np.asarray("euler"))
    x, P, y = FC.inputs(d0, gs)
    A, n = A_list[2], ns[2]
    make = lambda: single.ODEBlock(maxTime, deltaT, n, [0], H, single.ODEfunc(A, 0.2, 0.1, H, dev), dev)
    yt = torch.from_numpy(y.reshape(1, n, maxTime, 3)).to(torch.float64)
    d = _run(make, x, P, lambda S, I, R: ref_loss(helpers, S, I, R, yt, maxTime, deltaT))
    d.update(d0)
    np.savez_compressed(os.path.join(HERE, "input_grad_fbsocial_B1_H64_T30.npz"), **d)
    print("wrote fbsocial loss", d["loss"], "rest", d["rest_max"], "fp32 yardstick", _yard(d))
    # eight real graphs at H = 8 (composition A of real_multi_*), configs[4]
    H, maxTime = 8, 20
    d0 = dict(picks=np.asarray([4, 2, 3, 1, 0, 4, 2, 3], dtype=np.int32), H=np.int32(H), maxTime=np.int32(maxTime),
              deltaT=np.float64(deltaT), param_seed=np.int32(62), sample_seed=np.int32(6200), beta_scale=np.float64(0.03),
              method=np.asarray("euler"))
    x, P, y = FC.inputs(d0, gs)
    make = lambda: multi.ODEBlock(maxTime, deltaT, H, multi.ODEfunc(A_list, H, dev), dev)
    yt = torch.from_numpy(y).to(torch.float64)
    d = _run(make, x, P, lambda S, I, R: multi_loss(helpers, S, I, R, yt, maxTime, deltaT))
    d.update(d0)
    np.savez_compressed(os.path.join(HERE, "input_grad_multi8_H8_T20.npz"), **d)
    print("wrote multi8 loss", d["loss"], "rest", d["rest_max"], "fp32 yardstick", _yard(d))


if __name__ == "__main__":
    main()
