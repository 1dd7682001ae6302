#!/usr/bin/env python3
"""The exact gradient of the Euler solve (ops.backward adjoint=False; include/gnode.h gnode_backward_discrete_keep_f32) against
the adjoint backward, device-event timings after warm-up, one JSON line per shape:
  adjoint_ms     the adjoint's one-launch-per-interval form on a trajectory without keep (GNODE_FWD_PER_STEP): its twin
  exact_ms       the exact gradient on the recomputing form (a trajectory without keep, persist off), parameters only
  exact_dx_ms    parameters and x
  train_ms       the adjoint's default training backward (kept activations / persistent sweeps where they apply)
  exact_fast_ms  the exact gradient's default (ODEBlock(adjoint=False)): over the kept activations / one persistent launch,
                 exact_path = the form it takes (ops.discrete_path)
  *_per_iv_us    the same per interval; exact_over_adjoint, exact_over_train, exact_fast_over_train, exact_fast_over_exact:
                 the ratios DESIGN.md section 7.3 records
Run on the GPU:  python tools/bench_discrete_grad.py"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gn-ode-sir_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
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
    nint = len(dts)
    out = {"case": tag, "rows": rows, "H": H, "intervals": nint}
    _, _, _, sol_k = ops.forward(graph, x2d, P, dts, "euler", rows_out, want_sol=True)
    out["train_ms"] = ev_ms(lambda: ops.backward(graph, x2d, P, dts, "euler", rows_out, sol_k, gS, gI, gR))
    keep = sol_k.gnode_keep
    out["exact_path"] = ops.discrete_path(graph, rows, H, nint, rows_out, sol_k, keep)
    out["exact_fast_ms"] = ev_ms(lambda: ops.backward(graph, x2d, P, dts, "euler", rows_out, sol_k, gS, gI, gR, keep=keep, adjoint=False))
    del sol_k, keep
    _, _, _, sol = ops.forward(graph, x2d, P, dts, "euler", rows_out, want_sol=True, want_keep=False)
    bw = lambda **kw: ops.backward(graph, x2d, P, dts, "euler", rows_out, sol, gS, gI, gR, **kw)
    out["adjoint_ms"] = ev_ms(lambda: bw(keep=None, persist=False))
    out["exact_ms"] = ev_ms(lambda: bw(adjoint=False, persist=False))
    out["exact_dx_ms"] = ev_ms(lambda: bw(adjoint=False, want_x=True))
    for k in ("adjoint", "exact", "exact_dx"):
        out[k + "_per_iv_us"] = 1e3 * out[k + "_ms"] / nint
    out["exact_over_adjoint"] = out["exact_ms"] / out["adjoint_ms"]
    out["exact_over_train"] = out["exact_ms"] / out["train_ms"]
    out["exact_fast_over_train"] = out["exact_fast_ms"] / out["train_ms"]
    out["exact_fast_over_exact"] = out["exact_fast_ms"] / out["exact_ms"]
    print(json.dumps({k: round(v, 4) if isinstance(v, float) else v for k, v in out.items()}), flush=True)


def single(tag, rp, ci, B, H, maxTime):
    n = rp.shape[0] - 1
    x = torch.from_numpy(synth.samples(n, B, H, seed=1)).to(dev).reshape(B * n, 3 + H).contiguous()
    case(tag, DeviceGraph(rp, ci), x, H, maxTime)


def main():
    import fixture_cases as FC
    gs = FC.graphs()
    single("er75k_B4_H64_T30", *synth.er_csr(75000, 1000000 // 2, seed=0), 4, 64, 30)
    single("fbsocial_B1_H64_T30", *gs[2], 1, 64, 30)
    single("fbsocial_B1_H128_T30", *gs[2], 1, 128, 30)
    from gnode import ode_nn_ngraphs as multi
    x, _, _ = FC.inputs(FC.load("input_grad_multi8_H8_T20"), gs)         # the eight-graph training batch, 24 410 nodes
    x2d = torch.from_numpy(x).to(dev).contiguous()
    import scipy.sparse as sp
    adj = [sp.csr_matrix((np.ones(c.shape[0]), c, r), shape=(r.shape[0] - 1,) * 2) for r, c in gs]
    f = multi.ODEfunc(adj, 8, dev)
    case("multi8_H8_T20", f.graph_for(x2d[:, 5]), x2d, 8, 20)


if __name__ == "__main__":
    main()
