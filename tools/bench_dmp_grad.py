#!/usr/bin/env python3
"""The DMP gradient for 16 samples on one graph, at the shapes of tools/bench_dmp_batch.py: the backward of one `dmp_marginals`
call (gnode_dmp_batch_backward_f32: the forward again onto the tape, then the reverse sweep; all three gradients, per-sample
weights and gammas) against the forward of the same call (gnode_dmp_batch_f32).  Device tensors on both sides, the graph handle
made once; every timed call ends in a device synchronise.  One JSON line per graph, appended to
profiles/dmp_grad_bench.jsonl when --out is given; no threshold."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gn-ode-sir_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np, scipy.sparse as sp, torch
import gnode_oracle as O
from gnode import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="append the lines to this file as well")
ap.add_argument("--lib", default=None, help="load this build of libgnode_hip.so instead of the package's (as tools/bench_dmp_batch.py)")
opt = ap.parse_args()
if opt.lib:
    _lib.LIB_PATH = os.path.abspath(opt.lib)
from gnode.dmp import DmpGraph, dmp_marginals

SAMPLES, T = 16, 30


def timed(fn, reps=7):
    """Median wall-clock seconds of `reps` calls after a warm-up; every call ends in a device synchronise."""
    fn(); torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn(); torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times))


dev = torch.device("cuda:0")
for name, n, m in (("karate-size", 34, 78), ("er150-size", 150, 700), ("fb-social-size", 4039, 88234)):
    rp, ci, _ = O.er_graph(n, m, seed=1)
    G = DmpGraph(sp.csr_matrix((np.ones(len(ci)), ci, rp), shape=(n, n)))
    rng = np.random.default_rng(2)
    init = np.zeros((SAMPLES, n, 3), dtype=np.float32)
    init[:, :, 0] = 1.0
    for b in range(SAMPLES):
        init[b, rng.choice(n, size=2, replace=False)] = (0.0, 1.0, 0.0)
    scale = 0.5 / max(1.0, len(ci) / n)
    w = torch.full((SAMPLES, len(ci)), scale, dtype=torch.float32, device=dev, requires_grad=True)
    gam = torch.full((SAMPLES, n), 0.3, dtype=torch.float32, device=dev, requires_grad=True)
    y0 = torch.from_numpy(init).to(dev).requires_grad_(True)
    grad_out = torch.from_numpy(np.random.default_rng(0).standard_normal((SAMPLES, T, n, 3)).astype(np.float32)).to(dev)
    lib, handle = _lib.load(), G.graph.handle

    def forward():
        with torch.no_grad():
            return dmp_marginals(G, w, gam, y0, T)

    out = dmp_marginals(G, w, gam, y0, T)

    def backward():
        return torch.autograd.grad(out, (w, gam, y0), grad_out, retain_graph=True)

    t_fwd, t_bwd = timed(forward), timed(backward)
    first, again = backward(), backward()
    line = json.dumps({"case": name, "n": n, "nnz": int(len(ci)), "T": T, "samples": SAMPLES,
                       "forward_lds_bytes": int(lib.gnode_dmp_batch_lds_bytes(handle)),
                       "backward_lds_bytes": int(lib.gnode_dmp_batch_backward_lds_bytes(handle)),
                       "backward_workspace_bytes": int(lib.gnode_dmp_batch_backward_workspace_bytes(handle, SAMPLES, T)),
                       "forward_ms": t_fwd * 1e3, "backward_ms": t_bwd * 1e3, "backward_over_forward": t_bwd / t_fwd,
                       "finite": bool(all(torch.isfinite(g).all() for g in first)),
                       "deterministic": bool(all(torch.equal(a, b) for a, b in zip(first, again)))})
    print(line, flush=True)
    if opt.out:
        with open(opt.out, "a") as f:
            f.write(line + "\n")
