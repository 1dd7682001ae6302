#!/usr/bin/env python3
"""Monte-Carlo nowcast and forecast from timed evidence with every node a candidate: `posterior_states_mc` (one launch of C x sims
trajectories that decides acceptance on chip, ends the rejected ones at step `now` and counts the states of the accepted ones at
now + h) against the way a user had before it -- a loop over the candidates of `sir_trajectories(graph, InitialState with row c
replaced, ..., events=True)`, then the definition of a matched record on the event tensors and `sir_state_at` in torch, on one
graph handle -- and next to `source_scores_timed_mc` (the same trajectories, all of them run to T, tallied over every age: the
floor of what deciding acceptance costs) and `outbreak_sizes_mc` (the same trajectories without any tally) on the same inputs.
sims 1 000, T 30, now 15, horizons (0, 3, 7), w = 0.5 / mean degree, gamma 0.3, the start everybody susceptible; two evidence
sets, each alone: "tight", about 20 records that 8 sensors report (onset, removal, state: `observations_from_events`) at `now`
of the trajectory of candidate 0 (of eight) that has spread furthest, half the sensors among the nodes it has reached, which few
trajectories satisfy, and "always", one kind-0 record further back than T, which all do -- the first shows what ending rejected
jobs saves, the second what the 64-bit count atomics cost; karate (n 34) and the fb-social-size ER graph (n 1 893, nnz 27 670).
The two sides must agree integer for integer before a time is reported.
Median / minimum / maximum of REPS alternating calls after a warm-up of each, wall clock around a device synchronise.  One JSON
line per (graph, set), printed and appended to --out (profiles/sir_post_bench.jsonl by default).  No threshold."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gn-ode-sir_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np, torch
import gnode_oracle as O_
from gnode import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sir_post_bench.jsonl"))
ap.add_argument("--label", default="default")
ap.add_argument("--lib", default=None)
ap.add_argument("--graphs", default="karate,fb-social-size")
ap.add_argument("--sets", default="tight,always")
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
if args.lib:
    _lib.LIB_PATH = os.path.abspath(args.lib)
from gnode.dmp import observations_from_events, timed_observations
from gnode.graph import DeviceGraph
from gnode.ode_nn import (InitialState, _csr_from_edges, _edge_arrays, edge_rates, outbreak_sizes_mc, posterior_states_mc, sir_state_at,
                          sir_trajectories, source_scores_timed_mc)

SIMS, T, NOW, HORIZONS, GAMMA, RNG, SENSORS = 1000, 30, 15, (0, 3, 7), 0.3, 12345, 8
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
    t_inf, t_rec = first.t_inf.cpu().numpy(), first.t_rec.cpu().numpy()
    dev = first.t_inf.device
    for which in args.sets.split(","):
        if which == "tight":
            # the trajectory of the eight that has infected most by `now`; half the sensors among the nodes it has reached
            src = int(((t_inf >= 0) & (t_inf <= NOW)).sum(1).argmax())
            reached = np.flatnonzero((t_inf[src] >= 0) & (t_inf[src] <= NOW))[:SENSORS // 2].tolist()
            spread = [v for v in ((1 + i * (n // SENSORS)) % n for i in range(SENSORS)) if v not in reached]
            sensors = sorted(reached + spread[:SENSORS - len(reached)])
            rec = list(zip(*observations_from_events(t_inf[src], t_rec[src], NOW, sensors, what=("onset", "removal", "state"))))
        else:
            rec = [(0, -(T + 3), 0)]
        obs = timed_observations(n, *zip(*rec))
        node, off, kind = (torch.tensor([x[j] for x in rec], device=dev) for j in range(3))

        def fused():
            r = posterior_states_mc(g, obs, beta, GAMMA, SIMS, T, NOW, HORIZONS, rng_seed=RNG)
            return r.counts, r.accepted

        def scores():
            return source_scores_timed_mc(g, obs, beta, GAMMA, SIMS, T, bins=len(rec), rng_seed=RNG).hist

        def sizes():
            return outbreak_sizes_mc(g, beta, GAMMA, SIMS, T, action="seed", rng_seed=RNG).sums

        def loop():
            counts = torch.zeros((1, len(HORIZONS), 2, n), dtype=torch.int64, device=dev)
            accepted = torch.zeros((1, n), dtype=torch.int64, device=dev)
            m = (NOW + off)[None, :]                                                              # [1, R]
            for c in range(n):
                r = sir_trajectories(g, InitialState.from_sets(n, [c]), beta, GAMMA, SIMS, T, rng_seed=RNG, events=True, curves=False)
                a, b = r.t_inf.long()[:, node], r.t_rec.long()[:, node]                           # [sims, R]
                inf, rcv = (a >= 0) & (a <= m), (b >= 0) & (b <= m)
                k2 = kind[None, :]
                at = torch.where(k2 == 0, ~inf, torch.where(k2 == 1, inf & ~rcv, torch.where(k2 == 2, rcv, torch.where(k2 == 3, a == m, b == m))))
                ok = torch.where(m < 0, (k2 == 0).expand_as(at), at).all(1)                       # [sims]
                accepted[0, c] = ok.sum()
                for j, h in enumerate(HORIZONS):
                    st = sir_state_at(r.t_inf[ok], r.t_rec[ok], NOW + h)
                    counts[0, j, 0] += (st == 1).sum(0)
                    counts[0, j, 1] += (st == 2).sum(0)
            return counts, accepted

        got, want = run(fused)[1], run(loop)[1]                     # the warm-up of each, and the comparison
        hist, sums = run(scores)[1], run(sizes)[1]
        assert all(a.dtype == b.dtype == torch.int64 and torch.equal(a, b) for a, b in zip(got, want)), f"{name}, {which}: the fused counts are not the loop's"
        assert torch.equal(got[1][0], hist[0, :, NOW, len(rec)]), f"{name}, {which}: accepted is not the timed scores' top bin at now"
        if which == "always":
            assert all(torch.equal(got[0][0, j].sum(-1), sums[:, NOW + h, 1:3].sum(0)) for j, h in enumerate(HORIZONS)), f"{name}: the sizes' identity"
        times = {"fused": [], "loop": [], "scores": [], "sizes": []}
        for _ in range(args.reps):
            times["fused"].append(run(fused)[0])
            times["scores"].append(run(scores)[0])
            times["sizes"].append(run(sizes)[0])
            times["loop"].append(run(loop)[0])
        stat = lambda v: {"median": float(np.median(v)) * 1e3, "min": float(np.min(v)) * 1e3, "max": float(np.max(v)) * 1e3}      # noqa: E731
        line = json.dumps({"case": name, "build": args.label, "n": n, "nnz": int(nnz), "T": T, "sims": SIMS, "candidates": n, "set": which,
                           "records": len(rec), "now": NOW, "horizons": list(HORIZONS), "trajectories": n * SIMS, "equal": True,
                           "accepted": int(got[1].sum()), "posterior_states_mc_ms": stat(times["fused"]),
                           "source_scores_timed_mc_ms": stat(times["scores"]), "outbreak_sizes_mc_ms": stat(times["sizes"]),
                           "sir_trajectories_loop_ms": stat(times["loop"])})
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
