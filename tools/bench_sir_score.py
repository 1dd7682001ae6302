#!/usr/bin/env python3
"""Monte-Carlo source scores with every node a candidate: `source_scores_mc` (one launch of C x sims trajectories that leaves
the integer histogram of binned similarities) against the way a user had before it -- a loop over the candidates of
`sir_trajectories(graph, InitialState with row c replaced, ..., events=True)`, then per step `sir_state_at`, the same integer
bins in torch and `bincount`, on one graph handle -- and next to `outbreak_sizes_mc` on the same inputs (the same trajectories
without the tallies).  sims 1 000, T 30, w = 0.5 / mean degree, gamma 0.3, the start everybody susceptible, "jaccard", 64 bins;
O = 1 and O = 8 snapshots taken from trajectories of candidate 0 (step 3 + 3 o, every (o + 2)-th node hidden from o = 1 on);
karate (n 34) and the fb-social-size ER graph (n 1 893, nnz 27 670).  The two sides must agree integer for integer before a
time is reported.  Median / minimum / maximum of REPS alternating calls after a warm-up of each, wall clock around a device
synchronise.  One JSON line per (graph, O), printed and appended to --out (profiles/sir_score_bench.jsonl by default).  No
threshold."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gn-ode-sir_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np, torch
import gnode_oracle as O_
from gnode import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sir_score_bench.jsonl"))
ap.add_argument("--label", default="default")
ap.add_argument("--lib", default=None)
ap.add_argument("--graphs", default="karate,fb-social-size")
ap.add_argument("--snapshots", default="1,8")
args = ap.parse_args()
if args.lib:
    _lib.LIB_PATH = os.path.abspath(args.lib)
from gnode.graph import DeviceGraph
from gnode.ode_nn import (InitialState, _csr_from_edges, _edge_arrays, edge_rates, outbreak_sizes_mc, sir_state_at, sir_trajectories,
                          source_scores_mc)

SIMS, T, GAMMA, RNG, REPS, BINS, MEASURE = 1000, 30, 0.3, 12345, 7, 64, "jaccard"
assert torch.cuda.is_available(), "this measurement needs the GPU"


def graphs():
    import networkx as nx
    G = nx.karate_club_graph()
    yield ("karate", *_csr_from_edges(34, _edge_arrays(G)))
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
    for O in (int(x) for x in args.snapshots.split(",")):
        obs = torch.stack([sir_state_at(first.t_inf[o:o + 1], first.t_rec[o:o + 1], 3 + 3 * o)[0] for o in range(O)])
        for o in range(1, O):
            obs[o, ::o + 2] = -1
        seen = obs >= 0                                             # [O, n]
        marked = obs >= 1

        def fused():
            return source_scores_mc(g, obs, beta, GAMMA, SIMS, T, measure=MEASURE, bins=BINS, rng_seed=RNG).hist

        def sizes():
            return outbreak_sizes_mc(g, beta, GAMMA, SIMS, T, action="seed", rng_seed=RNG).sums

        def loop():
            hist = torch.zeros((O, n, T, BINS + 1), dtype=torch.int64, device=obs.device)
            shift = (torch.arange(O, device=obs.device) * (BINS + 1))[:, None]
            for c in range(n):
                r = sir_trajectories(g, InitialState.from_sets(n, [c]), beta, GAMMA, SIMS, T, rng_seed=RNG, events=True, curves=False)
                for t in range(T):
                    left = (sir_state_at(r.t_inf, r.t_rec, t) != 0)[None, :, :] & seen[:, None, :]      # [O, sims, n]
                    num = (left & marked[:, None, :]).sum(2)
                    den = (left | marked[:, None, :]).sum(2)
                    k = torch.where(den == 0, torch.full_like(num, BINS), (num * BINS) // den.clamp(min=1))
                    hist[:, c, t] = torch.bincount((k + shift).reshape(-1), minlength=O * (BINS + 1)).view(O, BINS + 1)
            return hist

        got, want = run(fused)[1], run(loop)[1]                     # the warm-up of each, and the comparison
        run(sizes)
        assert got.dtype == want.dtype == torch.int64 and torch.equal(got, want), f"{name}, O = {O}: the fused histogram is not the loop's"
        times = {"fused": [], "loop": [], "sizes": []}
        for _ in range(REPS):
            times["fused"].append(run(fused)[0])
            times["sizes"].append(run(sizes)[0])
            times["loop"].append(run(loop)[0])
        stat = lambda v: {"median": float(np.median(v)) * 1e3, "min": float(np.min(v)) * 1e3, "max": float(np.max(v)) * 1e3}      # noqa: E731
        line = json.dumps({"case": name, "build": args.label, "n": n, "nnz": int(nnz), "T": T, "sims": SIMS, "candidates": n, "snapshots": O,
                           "measure": MEASURE, "bins": BINS, "trajectories": n * SIMS, "equal": True, "source_scores_mc_ms": stat(times["fused"]),
                           "outbreak_sizes_mc_ms": stat(times["sizes"]), "sir_trajectories_loop_ms": stat(times["loop"]),
                           "top_bin_share": float(got[..., BINS].sum()) / float(O * n * T * SIMS)})
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
