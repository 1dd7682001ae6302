#!/usr/bin/env python3
"""Monte-Carlo outbreak sizes with every node a candidate: `outbreak_sizes_mc` (one launch of C x sims trajectories that leaves
the integer sums) against the way a user had before it -- a loop over the candidates of `sir_trajectories(graph, InitialState
with row c replaced, ..., events=False, curves=True).curves.sum(0)` on one graph handle.  sims 1 000, T 30, w = 0.5 / mean
degree, gamma 0.3, the start everybody susceptible, action "seed"; karate (n 34) and the fb-social-size ER graph (n 1 893, nnz
27 670).  The two sides must agree integer for integer before a time is reported.  Median / minimum / maximum of REPS
alternating calls after a warm-up of each, wall clock around a device synchronise.  One JSON line per graph, printed and
appended to --out (profiles/sir_sweep_bench.jsonl by default); --label names the build in the line; --lib loads another build
of the library (the job order is a compile-time choice, GN_SIR_SWEEP_MAJOR).  No threshold."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gn-ode-sir_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np, torch
import gnode_oracle as O
from gnode import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sir_sweep_bench.jsonl"))
ap.add_argument("--label", default="interleaved")
ap.add_argument("--lib", default=None)
ap.add_argument("--graphs", default="karate,fb-social-size")
args = ap.parse_args()
if args.lib:
    _lib.LIB_PATH = os.path.abspath(args.lib)
from gnode.graph import DeviceGraph
from gnode.ode_nn import InitialState, _csr_from_edges, _edge_arrays, edge_rates, outbreak_sizes_mc, sir_trajectories

SIMS, T, GAMMA, RNG, REPS = 1000, 30, 0.3, 12345, 7
assert torch.cuda.is_available(), "this measurement needs the GPU"


def graphs():
    import networkx as nx
    G = nx.karate_club_graph()
    yield ("karate", *_csr_from_edges(34, _edge_arrays(G)))
    rp, ci, _ = O.er_graph(1893, 13835, seed=1)
    yield "fb-social-size", rp, ci


def run(fn):
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


for name, rp, ci in graphs():
    if name not in args.graphs.split(","):
        continue
    n, nnz = len(rp) - 1, len(ci)
    g = DeviceGraph(rp, ci)
    beta = edge_rates(g, np.full(nnz, 0.5 / max(1.0, nnz / n)))

    def fused():
        return outbreak_sizes_mc(g, beta, GAMMA, SIMS, T, action="seed", rng_seed=RNG).sums

    def loop():
        rows = []
        for c in range(n):
            cv = sir_trajectories(g, InitialState.from_sets(n, [c]), beta, GAMMA, SIMS, T, rng_seed=RNG, events=False, curves=True).curves
            rows.append(cv.sum(0, dtype=torch.int64))
        return torch.stack(rows)

    got, want = run(fused)[1], run(loop)[1]                         # the warm-up of each, and the comparison
    assert got.dtype == want.dtype == torch.int64 and torch.equal(got, want), f"{name}: the fused sums are not the loop's"
    times = {"fused": [], "loop": []}
    for _ in range(REPS):
        times["fused"].append(run(fused)[0])
        times["loop"].append(run(loop)[0])
    stat = lambda v: {"median": float(np.median(v)) * 1e3, "min": float(np.min(v)) * 1e3, "max": float(np.max(v)) * 1e3}      # noqa: E731
    line = json.dumps({"case": name, "build": args.label, "n": n, "nnz": int(nnz), "T": T, "sims": SIMS, "candidates": n,
                       "trajectories": n * SIMS, "equal": True, "outbreak_sizes_mc_ms": stat(times["fused"]),
                       "sir_trajectories_loop_ms": stat(times["loop"]),
                       "ever_infected_mean": float((got[:, -1, 1] + got[:, -1, 2] - got[:, 0, 2]).double().mean() / SIMS)})
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
