#!/usr/bin/env python3
"""Source inference with every node a candidate: `source_scores` (the likelihood sums fused into the DMP node pass) against the
composition a user had before it -- `dmp_batch` over the same candidates' seed lists in chunks of the same byte budget (counting
the marginals and the starts a chunk materialises), then torch.log(out.clamp(floor, 1).double()) gathered by `obs` and summed.
Both sides keep one `DmpGraph` (handle made before the timed region) and leave the [C, maxTime] table on the device.  Median /
minimum / maximum of REPS alternating calls after a warm-up of each, wall clock around a device synchronise; the peak of
torch's allocator during one call of each side (the library allocates nothing itself).  One JSON line per graph; no threshold."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gn-ode-sir_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np, scipy.sparse as sp, torch
import gnode_oracle as O
from gnode import _lib
from gnode.dmp import DmpGraph, dmp_batch, source_scores

T, FLOOR, BUDGET, REPS = 30, 1e-30, 1 << 30, 7
assert torch.cuda.is_available(), "this measurement needs the GPU"


def composed(G, obs_d, seen, gamma, cands):
    n = G.N
    chunk = max(1, BUDGET // ((T + 1) * n * 12))
    rows = []
    for at in range(0, len(cands), chunk):
        out = dmp_batch(G, [[int(c)] for c in cands[at:at + chunk]], gamma, T)
        logp = torch.log(out.clamp(float(np.float32(FLOOR)), 1.0).double())
        idx = obs_d[seen].view(1, 1, -1, 1).expand(out.shape[0], T, -1, 1)
        rows.append(logp[:, :, seen, :].gather(3, idx)[..., 0].sum(2))
        del out, logp
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
    obs = np.random.default_rng(3).choice(np.asarray([-1, 0, 1, 2]), size=n, p=[0.25, 0.35, 0.25, 0.15])
    lib, handle = _lib.load(), G.graph.handle
    obs_d = torch.from_numpy(obs).cuda()
    seen = torch.nonzero(obs_d >= 0).flatten()
    fused = lambda: source_scores(G, obs, gamma, T, candidates=cands, floor=FLOOR, budget_bytes=BUDGET)      # noqa: E731
    comp = lambda: composed(G, obs_d, seen, gamma, cands)                                                   # noqa: E731
    got, want = run(fused)[1], run(comp)[1]                         # the warm-up of each, and the comparison
    times = {"fused": [], "composed": []}
    for _ in range(REPS):
        times["fused"].append(run(fused)[0])
        times["composed"].append(run(comp)[0])
    n_obs = int(seen.numel())
    err = (got - want).abs()
    stat = lambda v: {"median": float(np.median(v)) * 1e3, "min": float(np.min(v)) * 1e3, "max": float(np.max(v)) * 1e3}      # noqa: E731
    print(json.dumps({"case": name, "n": n, "nnz": int(len(ci)), "T": T, "candidates": int(len(cands)), "observed": n_obs,
                      "budget_bytes": BUDGET, "source_lds_bytes": int(lib.gnode_dmp_source_lds_bytes(handle)),
                      "form": "one_workgroup" if lib.gnode_dmp_source_lds_bytes(handle) <= 160 * 1024 else "general",
                      "source_scores_ms": stat(times["fused"]), "dmp_batch_plus_torch_ms": stat(times["composed"]),
                      "source_scores_peak_bytes": peak_of(fused), "dmp_batch_plus_torch_peak_bytes": peak_of(comp),
                      "max_rel_diff": float((err / want.abs().clamp_min(1e-300)).max()),
                      "within_bar": bool((err <= (n_obs + 4) * 2.0 ** -52 * want.abs()).all()),
                      "same_ranking_head": bool(torch.equal(got.max(1).values.argsort(descending=True)[:5],
                                                            want.max(1).values.argsort(descending=True)[:5]))}), flush=True)
