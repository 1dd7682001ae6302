#!/usr/bin/env python3
"""The four outputs of the Monte-Carlo candidate sweep on the same inputs, the fused calls ALONE: `outbreak_sizes_mc`,
`source_scores_mc` (1 and 8 snapshots), `source_scores_timed_mc` (1 and 8 evidence sets) and `posterior_states_mc` (the "tight"
and the "always" set of bench_sir_post.py), every node a candidate, sims 1 000, T 30, w = 0.5 / mean degree, gamma 0.3, on the
frontier walk and (edge_scan) on the scan kernels; karate (n 34) and the fb-social-size ER graph (n 1 893, nnz 27 670).  The
bench_sir_{sweep,score,timed,post}.py tools time each call against the loop a user had before it, which takes minutes at
fb-social size; this one is for comparing two builds of the library (--lib, --label), where only the calls themselves matter.
Median / minimum / maximum of --reps calls after a warm-up, wall clock around a device synchronise; the frontier and scan results
of a call must be equal integer for integer.  One JSON line per (graph, call, path), printed and appended to --out.  No threshold."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gn-ode-sir_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np, torch
import gnode_oracle as O_
from gnode import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sir_outputs_bench.jsonl"))
ap.add_argument("--label", default="default")
ap.add_argument("--lib", default=None)
ap.add_argument("--graphs", default="karate,fb-social-size")
ap.add_argument("--calls", default="", help="comma-separated names of the calls to time (all by default)")
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
if args.lib:
    _lib.LIB_PATH = os.path.abspath(args.lib)
from gnode.dmp import observations_from_events, timed_observations
from gnode.graph import DeviceGraph
from gnode.ode_nn import (InitialState, _csr_from_edges, _edge_arrays, edge_rates, outbreak_sizes_mc, posterior_states_mc, sir_state_at,
                          sir_trajectories, source_scores_mc, source_scores_timed_mc)

SIMS, T, NOW, HORIZONS, GAMMA, RNG, SENSORS = 1000, 30, 15, (0, 3, 7), 0.3, 12345, 8
assert torch.cuda.is_available(), "this measurement needs the GPU"


def graphs():
    import networkx as nx
    yield ("karate", *_csr_from_edges(34, _edge_arrays(nx.karate_club_graph())))
    rp, ci, _ = O_.er_graph(1893, 13835, seed=1)
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
    first = sir_trajectories(g, InitialState.from_sets(n, [0]), beta, GAMMA, 8, T, rng_seed=RNG, events=True, curves=False)
    t_inf, t_rec = first.t_inf.cpu().numpy(), first.t_rec.cpu().numpy()
    snaps = torch.stack([sir_state_at(first.t_inf[o:o + 1], first.t_rec[o:o + 1], 3 + 3 * o)[0] for o in range(8)])
    for o in range(1, 8):
        snaps[o, ::o + 2] = -1
    sensors = [(1 + i * (n // SENSORS)) % n for i in range(SENSORS)]
    sets = [timed_observations(n, *observations_from_events(t_inf[o], t_rec[o], NOW, sensors, what=("onset", "removal", "state"))) for o in range(8)]
    always = timed_observations(n, [0], [-(T + 3)], [0])
    calls = {
        "sums": lambda es: outbreak_sizes_mc(g, beta, GAMMA, SIMS, T, action="seed", rng_seed=RNG, edge_scan=es).sums,
        "scores-1": lambda es: source_scores_mc(g, snaps[:1], beta, GAMMA, SIMS, T, rng_seed=RNG, edge_scan=es).hist,
        "scores-8": lambda es: source_scores_mc(g, snaps, beta, GAMMA, SIMS, T, rng_seed=RNG, edge_scan=es).hist,
        "timed-1": lambda es: source_scores_timed_mc(g, sets[:1], beta, GAMMA, SIMS, T, rng_seed=RNG, edge_scan=es).hist,
        "timed-8": lambda es: source_scores_timed_mc(g, sets, beta, GAMMA, SIMS, T, rng_seed=RNG, edge_scan=es).hist,
        "posterior-tight": lambda es: posterior_states_mc(g, sets[0], beta, GAMMA, SIMS, T, NOW, HORIZONS, rng_seed=RNG, edge_scan=es).counts,
        "posterior-always": lambda es: posterior_states_mc(g, always, beta, GAMMA, SIMS, T, NOW, HORIZONS, rng_seed=RNG, edge_scan=es).counts,
    }
    for call, fn in calls.items():
        if args.calls and call not in args.calls.split(","):
            continue
        walk, scan = run(lambda: fn(False))[1], run(lambda: fn(True))[1]      # the warm-up of each path, and the comparison
        assert torch.equal(walk, scan), f"{name}, {call}: the frontier walk and the scan disagree"
        for path, es in (("frontier", False), ("scan", True)):
            ms = [run(lambda: fn(es))[0] * 1e3 for _ in range(args.reps)]
            line = json.dumps({"case": name, "build": args.label, "call": call, "path": path, "n": n, "nnz": int(nnz), "T": T, "sims": SIMS,
                               "candidates": n, "checksum": int(walk.sum()),
                               "ms": {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}})
            print(line, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
