#!/usr/bin/env python3
"""Source inference from O snapshots with every node a candidate: `source_scores_batch` (one pass of the DMP recurrence, the O
likelihood sums taken in its node pass) against the loop a user had before it -- O `source_scores` calls on one `DmpGraph`,
stacked.  The snapshots are Monte-Carlo realisations from node 0, drawn on the GPU by `sir_trajectories` + `sir_state_at`; both
sides get the same int8 device table (the loop reads its rows back, as `source_scores` takes host input) and leave their
[O, C, maxTime] table on the device.  Median / minimum / maximum of REPS alternating calls after a warm-up of each, wall clock
around a device synchronise; the peak of torch's allocator during one call of each side (the library allocates nothing
itself); torch.equal of the two tables, and the mean rank of the true source.  One JSON line per (graph, O), printed and written to
profiles/dmp_source_batch_bench.jsonl; no threshold."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gn-ode-sir_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np, scipy.sparse as sp, torch
import gnode_oracle as O_
from gnode import _lib
from gnode.dmp import DmpGraph, source_rank_of, source_scores, source_scores_batch
from gnode.ode_nn import sir_state_at, sir_trajectories

T, FLOOR, BUDGET, REPS, SNAP_T, SOURCE = 30, 1e-30, 1 << 30, 5, 4, 0
OUT = os.path.join(ROOT, "profiles", "dmp_source_batch_bench.jsonl")
assert torch.cuda.is_available(), "this measurement needs the GPU"


def run(fn):
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def peak_of(fn):
    torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn(); torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


stat = lambda v: {"median": float(np.median(v)) * 1e3, "min": float(np.min(v)) * 1e3, "max": float(np.max(v)) * 1e3}      # noqa: E731
os.makedirs(os.path.dirname(OUT), exist_ok=True)
out_file = open(OUT, "w")
for name, n, m in (("karate-size", 34, 78), ("fb-social-size", 1893, 13835)):
    rp, ci, _ = O_.er_graph(n, m, seed=1)
    beta = 0.5 / max(1.0, len(ci) / n)
    G = DmpGraph(sp.csr_matrix((np.full(len(ci), beta), ci, rp), shape=(n, n)))
    gamma, cands = 0.3, np.arange(n)
    lib, handle = _lib.load(), G.graph.handle
    one_wg = lib.gnode_dmp_source_lds_bytes(handle) <= 160 * 1024
    tile = int(lib.gnode_dmp_source_batch_tile(handle))
    for O in (1, 8, 64):
        traj = sir_trajectories(G.graph, [SOURCE], beta, gamma, sims=O, T=SNAP_T + 1, rng_seed=3, curves=False)
        obs = sir_state_at(traj.t_inf, traj.t_rec, SNAP_T)              # int8 [O, n] on the device
        batch = lambda: source_scores_batch(G, obs, gamma, T, candidates=cands, floor=FLOOR, budget_bytes=BUDGET)      # noqa: E731
        loop = lambda: torch.stack([source_scores(G, row, gamma, T, candidates=cands, floor=FLOOR, budget_bytes=BUDGET)  # noqa: E731
                                    for row in obs.cpu().numpy()])
        got, want = run(batch)[1], run(loop)[1]                         # the warm-up of each, and the comparison
        times = {"batch": [], "loop": []}
        for _ in range(REPS):
            times["batch"].append(run(batch)[0])
            times["loop"].append(run(loop)[0])
        b, l = stat(times["batch"]), stat(times["loop"])
        line = json.dumps({"case": name, "n": n, "nnz": int(len(ci)), "T": T, "candidates": int(len(cands)), "O": O,
                           "form": "one_workgroup" if one_wg else "general", "tile": tile,
                           "recurrences_per_candidate": (O + tile - 1) // tile if one_wg else 1, "budget_bytes": BUDGET,
                           "source_scores_batch_ms": b, "source_scores_loop_ms": l, "loop_over_batch": l["median"] / b["median"],
                           "batch_beats_loop_by_more_than_its_spread": bool(l["median"] - b["median"] > l["max"] - l["min"]),
                           "source_scores_batch_peak_bytes": peak_of(batch), "source_scores_loop_peak_bytes": peak_of(loop),
                           "tables_equal": bool(torch.equal(got, want)),
                           "mean_rank_of_true_source": float(source_rank_of(got, cands, [SOURCE] * O).double().mean())})
        print(line, flush=True)
        out_file.write(line + "\n")
        out_file.flush()
