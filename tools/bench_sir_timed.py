#!/usr/bin/env python3
"""Monte-Carlo source scores from timed evidence with every node a candidate: `source_scores_timed_mc` (one launch of C x sims
trajectories that leaves the integer histogram of matched records per age) against the way a user had before it -- a loop over
the candidates of `sir_trajectories(graph, InitialState with row c replaced, ..., events=True)`, then the definition of a
matched record on the event tensors, the same integer bins in torch and `bincount`, on one graph handle -- and next to
`outbreak_sizes_mc` (the same trajectories without any tally) and `source_scores_mc` with as many snapshots as there are
evidence sets (the same trajectories with the per-step tally) on the same inputs.  sims 1 000, T 30, w = 0.5 / mean degree,
gamma 0.3, the start everybody susceptible; O = 1 and O = 8 evidence sets of about 20 records each, what 8 sensors report
(onset, removal, state: `observations_from_events`) at now = 6 + 2 o of trajectory o of candidate 0; karate (n 34) and the
fb-social-size ER graph (n 1 893, nnz 27 670).  The two sides must agree integer for integer before a time is reported.
Median / minimum / maximum of REPS alternating calls after a warm-up of each, wall clock around a device synchronise.  One JSON
line per (graph, O), printed and appended to --out (profiles/sir_timed_bench.jsonl by default); it also carries
`source_rank_of` of the true source under the Monte-Carlo's exact-match frequency, for the reader -- no test rests on it.  No
threshold."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gn-ode-sir_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np, torch
import gnode_oracle as O_
from gnode import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sir_timed_bench.jsonl"))
ap.add_argument("--label", default="default")
ap.add_argument("--lib", default=None)
ap.add_argument("--graphs", default="karate,fb-social-size")
ap.add_argument("--sets", default="1,8")
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
if args.lib:
    _lib.LIB_PATH = os.path.abspath(args.lib)
from gnode.dmp import observations_from_events, source_rank_of, timed_observations
from gnode.graph import DeviceGraph
from gnode.ode_nn import (InitialState, _csr_from_edges, _edge_arrays, edge_rates, outbreak_sizes_mc, sir_state_at, sir_trajectories,
                          source_scores_mc, source_scores_timed_mc)

SIMS, T, GAMMA, RNG, SENSORS = 1000, 30, 0.3, 12345, 8
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
    for O in (int(x) for x in args.sets.split(",")):
        sets, records = [], []
        for o in range(O):
            sensors = [(1 + o + i * (n // SENSORS)) % n for i in range(SENSORS)]
            rec = list(zip(*observations_from_events(t_inf[o], t_rec[o], 6 + 2 * o, sensors, what=("onset", "removal", "state"))))
            records.append(rec)
            sets.append(timed_observations(n, *zip(*rec)))
        bins = max(len(r) for r in records)
        dev = first.t_inf.device
        which = torch.tensor([o for o, r in enumerate(records) for _ in r], device=dev)
        node, off, kind = (torch.tensor([x[j] for r in records for x in r], device=dev) for j in range(3))
        size = torch.tensor([len(r) for r in records], device=dev)
        snaps = torch.stack([sir_state_at(first.t_inf[o:o + 1], first.t_rec[o:o + 1], 6 + 2 * o)[0] for o in range(O)])

        def fused():
            return source_scores_timed_mc(g, sets, beta, GAMMA, SIMS, T, bins=bins, rng_seed=RNG).hist

        def sizes():
            return outbreak_sizes_mc(g, beta, GAMMA, SIMS, T, action="seed", rng_seed=RNG).sums

        def snapshots():
            return source_scores_mc(g, snaps, beta, GAMMA, SIMS, T, measure="match", bins=bins, rng_seed=RNG).hist

        def loop():
            hist = torch.zeros((O, n, T, bins + 1), dtype=torch.int64, device=dev)
            shift = (torch.arange(O, device=dev) * (bins + 1))[:, None]
            m = (torch.arange(T, device=dev)[None, :] + off[:, None])[None, :, :]                # [1, R, T]
            for c in range(n):
                r = sir_trajectories(g, InitialState.from_sets(n, [c]), beta, GAMMA, SIMS, T, rng_seed=RNG, events=True, curves=False)
                a, b = r.t_inf.long()[:, node][:, :, None], r.t_rec.long()[:, node][:, :, None]   # [sims, R, 1]
                inf, rec = (a >= 0) & (a <= m), (b >= 0) & (b <= m)
                k3 = kind[None, :, None]
                at = torch.where(k3 == 0, ~inf, torch.where(k3 == 1, inf & ~rec, torch.where(k3 == 2, rec, torch.where(k3 == 3, a == m, b == m))))
                hit = torch.where(m < 0, (k3 == 0).expand_as(at), at).long()                      # [sims, R, T]
                agree = torch.zeros((SIMS, O, T), dtype=torch.int64, device=dev).index_add_(1, which, hit)
                k = (agree * bins) // size[None, :, None]                                         # [sims, O, T]
                for t in range(T):
                    hist[:, c, t] = torch.bincount((k[:, :, t].T + shift).reshape(-1), minlength=O * (bins + 1)).view(O, bins + 1)
            return hist

        got, want = run(fused)[1], run(loop)[1]                     # the warm-up of each, and the comparison
        run(sizes); run(snapshots)
        assert got.dtype == want.dtype == torch.int64 and torch.equal(got, want), f"{name}, O = {O}: the fused histogram is not the loop's"
        times = {"fused": [], "loop": [], "sizes": [], "snapshots": []}
        for _ in range(args.reps):
            times["fused"].append(run(fused)[0])
            times["sizes"].append(run(sizes)[0])
            times["snapshots"].append(run(snapshots)[0])
            times["loop"].append(run(loop)[0])
        # for the reader: where the true source (node 0) lands under the exact-match frequency, per evidence set
        mc = torch.log(torch.clamp(got[..., bins].double() / SIMS, min=1e-30))
        rank_mc = source_rank_of(mc, list(range(n)), [0] * O).tolist()
        stat = lambda v: {"median": float(np.median(v)) * 1e3, "min": float(np.min(v)) * 1e3, "max": float(np.max(v)) * 1e3}      # noqa: E731
        line = json.dumps({"case": name, "build": args.label, "n": n, "nnz": int(nnz), "T": T, "sims": SIMS, "candidates": n, "sets": O,
                           "records": [len(r) for r in records], "bins": bins, "trajectories": n * SIMS, "equal": True,
                           "source_scores_timed_mc_ms": stat(times["fused"]), "outbreak_sizes_mc_ms": stat(times["sizes"]),
                           "source_scores_mc_ms": stat(times["snapshots"]), "sir_trajectories_loop_ms": stat(times["loop"]),
                           "top_bin_share": float(got[..., bins].sum()) / float(O * n * T * SIMS), "rank_of_truth_mc": rank_mc})
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
