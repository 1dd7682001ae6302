#!/usr/bin/env python3
"""The mean-field gradient for 16 samples on one graph: forward + backward of one `meanfield_marginals` call
(gnode_meanfield_rates_steps_f64, then gnode_meanfield_rates_backward_f64: every interval integrated again from the recorded
steps, then swept in reverse; all four gradients, per-sample beta and gamma, a shared table of contact weights) against the
forward alone, at er150 size and at fb-social size.  Device tensors on both sides, the graph handle made once; every timed call
ends in a device synchronise.  The launches per accepted step are counted from the record: 6 for the integration, 7 for the
reverse and 5 for recomputing the stages of every step but an interval's last; the forward has 13 kernel launches per
attempted step.  One JSON line per graph, appended to profiles/meanfield_grad_bench.jsonl when --out is given; no threshold."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gn-ode-sir_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np, torch
import gnode_oracle as O
from gnode import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="append the lines to this file as well")
ap.add_argument("--lib", default=None, help="load this build of libgnode_hip.so instead of the package's (as tools/bench_dmp_grad.py)")
opt = ap.parse_args()
if opt.lib:
    _lib.LIB_PATH = os.path.abspath(opt.lib)
from gnode.graph import DeviceGraph
from gnode.ode_nn import meanfield_marginals

SAMPLES, T = 16, 30


def timed(fn, reps=5):
    """Median wall-clock seconds of `reps` calls after a warm-up; every call ends in a device synchronise."""
    fn(); torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn(); torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times))


dev = torch.device("cuda:0")
for name, n, m in (("er150-size", 150, 700), ("fb-social-size", 4039, 88234)):
    rp, ci, _ = O.er_graph(n, m, seed=1)
    G = DeviceGraph(rp, ci)
    rng = np.random.default_rng(2)
    init = np.zeros((SAMPLES, n, 3))
    init[:, :, 0] = 1.0
    for b in range(SAMPLES):
        init[b, rng.choice(n, size=2, replace=False)] = (0.0, 1.0, 0.0)
    scale = 0.5 / max(1.0, len(ci) / n)
    f = dict(dtype=torch.float64, device=dev)
    w = torch.full((len(ci),), scale, requires_grad=True, **f)
    beta = torch.from_numpy(rng.uniform(0.8, 1.2, (SAMPLES, n))).to(dev).requires_grad_(True)
    gam = torch.full((SAMPLES, n), 0.3, requires_grad=True, **f)
    y0 = torch.from_numpy(init).to(dev).requires_grad_(True)
    gout = [torch.from_numpy(np.random.default_rng(k).standard_normal((SAMPLES, T, n))).to(dev) for k in range(3)]

    def forward():
        with torch.no_grad():
            return meanfield_marginals(G, y0, beta, gam, w, maxTime=T)

    def both():
        out = meanfield_marginals(G, y0, beta, gam, w, maxTime=T)
        return torch.autograd.grad(out, (y0, beta, gam, w), gout)

    t_fwd, t_both = timed(forward), timed(both)
    first, again = both(), both()
    ctx = meanfield_marginals(G, y0, beta, gam, w, maxTime=T).I.grad_fn          # the record of the accepted steps
    n_acc, n_h = ctx.n_acc, int(ctx.h.shape[0])
    intervals = int((n_acc > 0).sum())
    lib = _lib.load()
    line = json.dumps({"case": name, "n": n, "nnz": int(len(ci)), "T": T, "samples": SAMPLES, "accepted_steps": n_h,
                       "max_interval_steps": int(n_acc.max()),
                       "backward_workspace_bytes": int(lib.gnode_meanfield_rates_backward_workspace_bytes(G.handle, SAMPLES, int(n_acc.max()))),
                       "backward_launches_per_step": (18 * n_h - 5 * intervals) / n_h, "forward_launches_per_step": 13,
                       "forward_ms": t_fwd * 1e3, "forward_backward_ms": t_both * 1e3, "backward_ms": (t_both - t_fwd) * 1e3,
                       "backward_over_forward": (t_both - t_fwd) / t_fwd,
                       "finite": bool(all(torch.isfinite(g).all() for g in first)),
                       "deterministic": bool(all(torch.equal(a, b) for a, b in zip(first, again)))})
    print(line, flush=True)
    if opt.out:
        with open(opt.out, "a") as f_out:
            f_out.write(line + "\n")
