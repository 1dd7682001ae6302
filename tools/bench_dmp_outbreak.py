#!/usr/bin/env python3
"""One greedy immunisation round with every node a candidate: `outbreak_sizes(action="immunise")` (the sums over the nodes fused
into the DMP node pass) against the composition a user had before it -- `dmp_batch` over one `InitialState` per candidate (the
base start with that node's row replaced) in chunks of the same byte budget (counting the marginals and the starts a chunk
materialises), then out.double().sum(nodes).  Both sides keep one `DmpGraph` (handle made before the timed region) and leave the
[C, maxTime, 3] table on the device; the composed side's starts are built on the host inside the timed region, as a user's
round would build them.  Median / minimum / maximum of REPS alternating calls after a warm-up of each, wall clock around a
device synchronise; the peak of torch's allocator during one call of each side (the library allocates nothing itself).  One
JSON line per graph; no threshold."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gn-ode-sir_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np, scipy.sparse as sp, torch
import gnode_oracle as O
from gnode import _lib
from gnode.dmp import DmpGraph, dmp_batch, infections, outbreak_sizes
from gnode.ode_nn import InitialState

T, BUDGET, REPS = 30, 1 << 30, 7
assert torch.cuda.is_available(), "this measurement needs the GPU"


def composed(G, base, gamma, cands):
    n = G.N
    chunk = max(1, BUDGET // ((T + 1) * n * 12))
    rows = []
    for at in range(0, len(cands), chunk):
        starts = []
        for c in cands[at:at + chunk]:
            p = base.p.copy()
            p[c] = (0.0, 0.0, 1.0)
            starts.append(InitialState(p))
        out = dmp_batch(G, starts, gamma, T)
        rows.append(out.double().sum(2))
        del out
    return torch.cat(rows)


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


for name, n, m in (("karate-size", 34, 78), ("fb-social-size", 1893, 13835)):
    rp, ci, _ = O.er_graph(n, m, seed=1)
    G = DmpGraph(sp.csr_matrix((np.full(len(ci), 0.5 / max(1.0, len(ci) / n)), ci, rp), shape=(n, n)))
    gamma, cands = 0.3, np.arange(n)
    seeds = np.random.default_rng(3).choice(n, size=max(1, n // 20), replace=False)
    base = InitialState.from_sets(n, seeds)
    lib, handle = _lib.load(), G.graph.handle
    fused = lambda: outbreak_sizes(G, gamma, T, candidates=cands, action="immunise", start=base, budget_bytes=BUDGET)       # noqa: E731
    comp = lambda: composed(G, base, gamma, cands)                                                                         # noqa: E731
    got, want = run(fused)[1], run(comp)[1]                         # the warm-up of each, and the comparison
    times = {"fused": [], "composed": []}
    for _ in range(REPS):
        times["fused"].append(run(fused)[0])
        times["composed"].append(run(comp)[0])
    err = (got - want).abs()
    stat = lambda v: {"median": float(np.median(v)) * 1e3, "min": float(np.min(v)) * 1e3, "max": float(np.max(v)) * 1e3}      # noqa: E731
    print(json.dumps({"case": name, "n": n, "nnz": int(len(ci)), "T": T, "candidates": int(len(cands)), "seeds": int(len(seeds)),
                      "budget_bytes": BUDGET, "outbreak_lds_bytes": int(lib.gnode_dmp_outbreak_lds_bytes(handle)),
                      "form": "one_workgroup" if lib.gnode_dmp_outbreak_lds_bytes(handle) <= 160 * 1024 else "general",
                      "outbreak_sizes_ms": stat(times["fused"]), "dmp_batch_plus_torch_ms": stat(times["composed"]),
                      "outbreak_sizes_peak_bytes": peak_of(fused), "dmp_batch_plus_torch_peak_bytes": peak_of(comp),
                      "max_abs_diff": float(err.max()),
                      "within_bar": bool((err <= n * 2.0 ** -52 * want.abs()).all()),     # |sum| <= sum|.|: no looser than the tests' bar
                      "same_choice": bool(int(infections(got).argmin()) == int(infections(want).argmin()))}), flush=True)
