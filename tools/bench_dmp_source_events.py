#!/usr/bin/env python3
"""Source inference from time-stamped records with every node a candidate: `source_scores_events` (the five likelihood terms
formed in the DMP node pass, every row summed there) against the composition on `dmp_batch` -- the same candidates' seed lists in
chunks of the same byte budget (counting the marginals, their two shifted copies, the five float32 probabilities and their
float64 logarithms a chunk materialises), the float32 differences Ps(t-1) - Ps(t) and Pr(t) - Pr(t-1), the float32 clamp, the float64 logarithm, and the
masked sum per row.  The rows are what `timed_observations` packs from one Monte-Carlo trajectory from node 0 (the largest of 16
drawn by `sir_trajectories`), reported at step NOW by a third of the nodes as onset and removal times: one row per distinct offset.
Both sides keep one `DmpGraph` (handle made before the timed region) and leave the [R, C, maxTime] table on the device.  Median /
minimum / maximum of REPS alternating calls after a warm-up of each, wall clock around a device synchronise; the peak of
torch's allocator during one call of each side (the library allocates nothing itself); the largest difference of the two tables
against the derived bar (n_coded + 4) * 2^-52 * |composed|; `source_scores_timed` once more on top, and where it ranks the true
source.  One JSON line per graph, printed and written to profiles/dmp_source_events_bench.jsonl; no threshold."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gn-ode-sir_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np, scipy.sparse as sp, torch
import gnode_oracle as O
from gnode import _lib
from gnode.dmp import (DmpGraph, dmp_batch, observations_from_events, rank_sources, source_scores_events, source_scores_timed,
                       timed_observations)
from gnode.ode_nn import sir_trajectories

T, FLOOR, BUDGET, REPS, NOW, SOURCE = 30, 1e-30, 1 << 30, 7, 6, 0
OUT = os.path.join(ROOT, "profiles", "dmp_source_events_bench.jsonl")
assert torch.cuda.is_available(), "this measurement needs the GPU"


def composed(G, onehot, gamma, cands):
    """[R, C, T] float64; onehot [R, 5, n] float64 on the device: which of the five terms a row takes from a node, if any"""
    n = G.N
    chunk = max(1, BUDGET // (T * n * (12 + 2 * 4 + 5 * 4 + 5 * 8) + n * 12))      # marginals, the two shifted copies, five p, five logs
    floor = float(np.float32(FLOOR))
    tables = []
    for at in range(0, len(cands), chunk):
        out = dmp_batch(G, [[int(c)] for c in cands[at:at + chunk]], gamma, T)
        ps, pi, pr = out[..., 0], out[..., 1], out[..., 2]
        ps_prev = torch.cat([torch.ones_like(ps[:, :1]), ps[:, :-1]], 1)
        pr_prev = torch.cat([torch.zeros_like(pr[:, :1]), pr[:, :-1]], 1)
        logp = torch.stack([ps, pi, pr, ps_prev - ps, pr - pr_prev]).clamp_(floor, 1.0).double().log_()      # [5, c, T, n]
        tables.append(torch.einsum("rjk,jctk->rct", onehot, logp))
        del out, logp
    return torch.cat(tables, 1)


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
    rp, ci, _ = O.er_graph(n, m, seed=1)
    beta = 0.5 / max(1.0, len(ci) / n)
    G = DmpGraph(sp.csr_matrix((np.full(len(ci), beta), ci, rp), shape=(n, n)))
    gamma, cands = 0.3, np.arange(n)
    lib, handle = _lib.load(), G.graph.handle
    one_wg = lib.gnode_dmp_source_lds_bytes(handle) <= 160 * 1024
    traj = sir_trajectories(G.graph, [SOURCE], beta, gamma, sims=16, T=NOW + 1, rng_seed=3, curves=False)
    s = int((traj.t_inf >= 0).sum(1).argmax())                      # the largest of 16 outbreaks: one that did not die out at once
    sensors = np.arange(0, n, 3)
    records = observations_from_events(traj.t_inf[s], traj.t_rec[s], NOW, sensors, what=("onset", "removal"))
    obs = timed_observations(n, *records)
    rows = torch.from_numpy(obs.rows).cuda()
    onehot = torch.stack([(rows == code) for code in range(5)], 1).double()
    n_coded = (rows >= 0).sum(1).double().view(-1, 1, 1)
    fused = lambda: source_scores_events(G, rows, gamma, T, candidates=cands, floor=FLOOR, budget_bytes=BUDGET)      # noqa: E731
    comp = lambda: composed(G, onehot, gamma, cands)                                                                # noqa: E731
    got, want = run(fused)[1], run(comp)[1]                         # the warm-up of each, and the comparison
    times = {"fused": [], "composed": []}
    for _ in range(REPS):
        times["fused"].append(run(fused)[0])
        times["composed"].append(run(comp)[0])
    err = (got - want).abs()
    timed = run(lambda: source_scores_timed(G, obs, gamma, T, candidates=cands, floor=FLOOR, budget_bytes=BUDGET))
    ranked = [k for k, _, _ in rank_sources(timed[1], cands)]
    line = json.dumps({"case": name, "n": n, "nnz": int(len(ci)), "T": T, "candidates": int(len(cands)), "rows": int(len(obs.rows)),
                       "records": int(len(records[0])), "event_records": int(obs.row_events.sum()), "row_offsets": obs.row_offsets.tolist(),
                       "budget_bytes": BUDGET, "form": "one_workgroup" if one_wg else "general",
                       "tile": int(lib.gnode_dmp_source_events_tile(handle)),
                       "source_scores_events_ms": stat(times["fused"]), "dmp_batch_plus_torch_ms": stat(times["composed"]),
                       "composed_over_fused": float(np.median(times["composed"]) / np.median(times["fused"])),
                       "source_scores_events_peak_bytes": peak_of(fused), "dmp_batch_plus_torch_peak_bytes": peak_of(comp),
                       "max_rel_diff": float((err / want.abs().clamp_min(1e-300)).max()),
                       "within_bar": bool((err <= (n_coded + 4) * 2.0 ** -52 * want.abs()).all()),
                       "source_scores_timed_ms_once": timed[0] * 1e3, "rank_of_true_source_timed": int(ranked.index(SOURCE))})
    print(line, flush=True)
    out_file.write(line + "\n")
    out_file.flush()
