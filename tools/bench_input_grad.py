#!/usr/bin/env python3
"""One Euler adjoint backward with and without the input gradient (ops.backward want_x; include/gnode.h
gnode_backward_dx_f32), device-event timings after warm-up, one JSON line per shape:
  train_ms  the training backward on the training forward's trajectory (kept activations / persistent sweeps where they apply)
  recompute_ms  the parameter-only backward on a trajectory produced without keep, on the form a gx call takes
  dx_ms     parameters and x (the recomputing one-launch-per-interval forms)
  dx_only_ms  x alone (want_params=False: the frozen-model calibration case)
Run on the GPU:  python tools/bench_input_grad.py"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gn-ode-sir_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import gnode_oracle as O
from gnode import ops, synth
from gnode.graph import DeviceGraph

dev = torch.device("cuda:0")


def ev_ms(fn, reps=10):
    fn(); fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def case(tag, graph, x2d, H, maxTime, deltaT=0.5):
    P = {k: torch.from_numpy(v).to(dev) for k, v in synth.linear_params(H, seed=0).items()}
    dts = ops.step_sizes(ops.time_grid(maxTime, deltaT))
    rows_out = ops.subsample_rows(maxTime, deltaT)
    g = torch.Generator().manual_seed(1)
    rows = x2d.shape[0]
    gS, gI, gR = (torch.randn((len(rows_out), rows), generator=g).to(dev) for _ in range(3))
    out = {"case": tag, "rows": rows, "H": H, "intervals": len(dts)}
    _, _, _, sol_k = ops.forward(graph, x2d, P, dts, "euler", rows_out, want_sol=True)
    out["train_ms"] = ev_ms(lambda: ops.backward(graph, x2d, P, dts, "euler", rows_out, sol_k, gS, gI, gR))
    del sol_k
    _, _, _, sol = ops.forward(graph, x2d, P, dts, "euler", rows_out, want_sol=True, want_keep=False)
    out["recompute_ms"] = ev_ms(lambda: ops.backward(graph, x2d, P, dts, "euler", rows_out, sol, gS, gI, gR, keep=None, persist=False))
    out["dx_ms"] = ev_ms(lambda: ops.backward(graph, x2d, P, dts, "euler", rows_out, sol, gS, gI, gR, keep=None, want_x=True))
    out["dx_only_ms"] = ev_ms(lambda: ops.backward(graph, x2d, P, dts, "euler", rows_out, sol, gS, gI, gR, keep=None, want_x=True,
                                                   want_params=False))
    out["dx_over_train"] = out["dx_ms"] / out["train_ms"]
    out["dx_over_recompute"] = out["dx_ms"] / out["recompute_ms"]
    print(json.dumps({k: round(v, 4) if isinstance(v, float) else v for k, v in out.items()}), flush=True)


def single(tag, rp, ci, B, H, maxTime):
    n = rp.shape[0] - 1
    x = torch.from_numpy(synth.samples(n, B, H, seed=1)).to(dev).reshape(B * n, 3 + H).contiguous()
    case(tag, DeviceGraph(rp, ci), x, H, maxTime)


def main():
    d = np.load(os.path.join(ROOT, "tests", "golden", "input_grad_karate_B2_H64_T20.npz"))
    single("karate_B1_H64_T20", *O.csr_from_edges(int(d["n"]), d["edges"]), 1, 64, 20)
    single("fbsize_B8_H64_T30", *synth.er_csr(1893, 13835, seed=0), 8, 64, 30)
    single("er75k_B4_H64_T30", *synth.er_csr(75000, 1000000 // 2, seed=0), 4, 64, 30)
    import fixture_cases as FC
    from gnode import ode_nn_ngraphs as multi
    gs = FC.graphs()
    x, _, _ = FC.inputs(FC.load("input_grad_multi8_H8_T20"), gs)
    x2d = torch.from_numpy(x).to(dev).contiguous()
    import scipy.sparse as sp
    adj = [sp.csr_matrix((np.ones(c.shape[0]), c, r), shape=(r.shape[0] - 1,) * 2) for r, c in gs]
    f = multi.ODEfunc(adj, 8, dev)
    case("multi8_H8_T20", f.graph_for(x2d[:, 5]), x2d, 8, 20)


if __name__ == "__main__":
    main()
