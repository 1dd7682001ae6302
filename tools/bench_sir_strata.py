#!/usr/bin/env python3
"""Monte-Carlo nowcast from evidence that may be wrong with every node a candidate: `posterior_strata_mc` at mismatches M = 0, 1,
2, 4 (one launch of C x sims trajectories that keeps a trajectory in stratum d = the records it misses while d <= M, ends the
others at step `now` and counts the states per stratum at now + h) against `posterior_states_mc` in the same process (the
exact-match call, whose code this feature does not touch) and against the way a user had before either -- a loop over the
candidates of `sir_trajectories(graph, InitialState with row c replaced, ..., events=True)`, then the definition of a matched
record on the event tensors and `sir_state_at` in torch per stratum, on one graph handle.  The setup is
tools/bench_sir_post.py's: sims 1 000, T 30, now 15, horizons (0, 3, 7), w = 0.5 / mean degree, gamma 0.3, the start everybody
susceptible; two evidence sets, each alone: "tight", about 20 records that 8 sensors report at `now` of the trajectory of
candidate 0 (of eight) that has spread furthest, and "always", one kind-0 record further back than T; karate (n 34) and the
fb-social-size ER graph (n 1 893, nnz 27 670).  Every M must agree with the loop integer for integer, and M = 0 with
`posterior_states_mc`, before a time is reported.
Median / minimum / maximum of REPS alternating calls after a warm-up of each, wall clock around a device synchronise.  Per M: the
accepted total, by stratum, `.ess(error=0.05)` -- the number the strata exist to raise -- and the time.  One JSON line per
(graph, set), printed and appended to --out (profiles/sir_strata_bench.jsonl by default).  No threshold."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gn-ode-sir_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np, torch
import gnode_oracle as O_
from gnode import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sir_strata_bench.jsonl"))
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
from gnode.ode_nn import (InitialState, _csr_from_edges, _edge_arrays, edge_rates, posterior_states_mc, posterior_strata_mc, sir_state_at,
                          sir_trajectories)

SIMS, T, NOW, HORIZONS, GAMMA, RNG, SENSORS, MS, ERROR = 1000, 30, 15, (0, 3, 7), 0.3, 12345, 8, (0, 1, 2, 4), 0.05
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

        def exact():
            r = posterior_states_mc(g, obs, beta, GAMMA, SIMS, T, NOW, HORIZONS, rng_seed=RNG)
            return r.counts, r.accepted

        def strata(M):
            return posterior_strata_mc(g, obs, beta, GAMMA, SIMS, T, NOW, HORIZONS, M, rng_seed=RNG)

        def loop(M=max(MS)):
            D = M + 1
            counts = torch.zeros((1, D, len(HORIZONS), 2, n), dtype=torch.int64, device=dev)
            accepted = torch.zeros((1, n, D), dtype=torch.int64, device=dev)
            m = (NOW + off)[None, :]                                                              # [1, R]
            for c in range(n):
                r = sir_trajectories(g, InitialState.from_sets(n, [c]), beta, GAMMA, SIMS, T, rng_seed=RNG, events=True, curves=False)
                a, b = r.t_inf.long()[:, node], r.t_rec.long()[:, node]                           # [sims, R]
                inf, rcv = (a >= 0) & (a <= m), (b >= 0) & (b <= m)
                k2 = kind[None, :]
                at = torch.where(k2 == 0, ~inf, torch.where(k2 == 1, inf & ~rcv, torch.where(k2 == 2, rcv, torch.where(k2 == 3, a == m, b == m))))
                miss = len(rec) - torch.where(m < 0, (k2 == 0).expand_as(at), at).sum(1)          # [sims]
                for d in range(D):
                    ok = miss == d
                    accepted[0, c, d] = ok.sum()
                    for j, h in enumerate(HORIZONS):
                        st = sir_state_at(r.t_inf[ok], r.t_rec[ok], NOW + h)
                        counts[0, d, j, 0] += (st == 1).sum(0)
                        counts[0, d, j, 1] += (st == 2).sum(0)
            return counts, accepted

        post, want = run(exact)[1], run(loop)[1]                    # the warm-up of each, and the comparison
        per = {}
        for M in MS:
            r = run(lambda: strata(M))[1]
            assert r.counts.dtype == r.accepted.dtype == torch.int64, f"{name}, {which}, M = {M}: the outputs are not int64"
            assert torch.equal(r.counts, want[0][:, :M + 1]) and torch.equal(r.accepted, want[1][..., :M + 1]), f"{name}, {which}, M = {M}: the fused strata are not the loop's"
            per[M] = {"accepted": int(r.accepted.sum()), "by_stratum": r.by_stratum().tolist(), "ess": float(r.ess(error=ERROR)), "complete": bool(r.complete())}
        r0 = strata(0)
        assert torch.equal(r0.counts[:, 0], post[0]) and torch.equal(r0.accepted[..., 0], post[1]), f"{name}, {which}: stratum 0 is not posterior_states_mc"
        times = {"exact": [], "loop": [], **{M: [] for M in MS}}
        for _ in range(args.reps):
            times["exact"].append(run(exact)[0])
            for M in MS:
                times[M].append(run(lambda: strata(M))[0])
            times["loop"].append(run(loop)[0])
        stat = lambda v: {"median": float(np.median(v)) * 1e3, "min": float(np.min(v)) * 1e3, "max": float(np.max(v)) * 1e3}      # noqa: E731
        for M in MS:
            per[M]["ms"] = stat(times[M])
        line = json.dumps({"case": name, "build": args.label, "n": n, "nnz": int(nnz), "T": T, "sims": SIMS, "candidates": n, "set": which,
                           "records": len(rec), "now": NOW, "horizons": list(HORIZONS), "trajectories": n * SIMS, "equal": True, "error": ERROR,
                           "posterior_states_mc_ms": stat(times["exact"]), "posterior_strata_mc": {str(M): per[M] for M in MS},
                           "m0_over_posterior": float(np.median(times[0]) / np.median(times["exact"])),
                           "sir_trajectories_loop_ms": stat(times["loop"])})
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
