#!/usr/bin/env python3
"""The scheduled DMP gradient for 16 samples on one graph, at the shapes and by the method of tools/bench_dmp_grad.py (T = 30,
median of 7 calls after a warm-up, every call ends in a device synchronise): the backward of one `dmp_marginals_schedule` call
(gnode_dmp_batch_schedule_backward_f32: the table check, the forward again onto the tape, the reverse sweep; all three
gradients, per-sample tables) with ONE phase against the backward of `dmp_marginals` (gnode_dmp_batch_backward_f32) on the same
numbers in the same process, and with P = 4 phases visited in turn (phase[t] = (t - 1) % 4, so every edge pass writes two
tables).  The forwards of the three calls are timed next to them: the scheduled entries read their tables back to the host and
check them on every call, which the constant entries do not, and the forwards show what that costs.  One JSON line per graph, appended to profiles/dmp_schedule_grad_bench.jsonl when --out is given; no threshold."""
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
from gnode.dmp import DmpGraph, dmp_marginals, dmp_marginals_schedule

SAMPLES, T, PHASES = 16, 30, 4


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
    y0 = torch.from_numpy(init).to(dev).requires_grad_(True)
    grad_out = torch.from_numpy(np.random.default_rng(0).standard_normal((SAMPLES, T, n, 3)).astype(np.float32)).to(dev)
    lib, handle = _lib.load(), G.graph.handle

    def tables(P):
        w = torch.full((SAMPLES, P, len(ci)), scale, dtype=torch.float32, device=dev, requires_grad=True)
        gam = torch.full((SAMPLES, P, n), 0.3, dtype=torch.float32, device=dev, requires_grad=True)
        return w, gam

    w0 = torch.full((SAMPLES, len(ci)), scale, dtype=torch.float32, device=dev, requires_grad=True)
    g0 = torch.full((SAMPLES, n), 0.3, dtype=torch.float32, device=dev, requires_grad=True)
    out0 = dmp_marginals(G, w0, g0, y0, T)
    constant = lambda: torch.autograd.grad(out0, (w0, g0, y0), grad_out, retain_graph=True)      # noqa: E731
    w1, g1 = tables(1)
    out1 = dmp_marginals_schedule(G, w1, g1, y0, T, np.zeros(T, dtype=np.int32))
    one = lambda: torch.autograd.grad(out1, (w1, g1, y0), grad_out, retain_graph=True)           # noqa: E731
    w4, g4 = tables(PHASES)
    phase4 = np.concatenate([[0], np.arange(T - 1) % PHASES]).astype(np.int32)
    out4 = dmp_marginals_schedule(G, w4, g4, y0, T, phase4)
    four = lambda: torch.autograd.grad(out4, (w4, g4, y0), grad_out, retain_graph=True)          # noqa: E731
    t_fwd1 = timed(lambda: dmp_marginals_schedule(G, w1.detach(), g1.detach(), y0.detach(), T, np.zeros(T, dtype=np.int32)))
    t_fwd4 = timed(lambda: dmp_marginals_schedule(G, w4.detach(), g4.detach(), y0.detach(), T, phase4))
    t_fwd0 = timed(lambda: dmp_marginals(G, w0.detach(), g0.detach(), y0.detach(), T))
    t_const, t_one, t_four = timed(constant), timed(one), timed(four)
    a, b, c4, c4_again = constant(), one(), four(), four()
    line = json.dumps({"case": name, "n": n, "nnz": int(len(ci)), "T": T, "samples": SAMPLES, "phases": PHASES,
                       "backward_lds_bytes": int(lib.gnode_dmp_batch_backward_lds_bytes(handle)),
                       "schedule_backward_workspace_bytes": int(lib.gnode_dmp_batch_schedule_backward_workspace_bytes(handle, SAMPLES, T)),
                       "constant_forward_ms": t_fwd0 * 1e3, "one_phase_forward_ms": t_fwd1 * 1e3, "four_phase_forward_ms": t_fwd4 * 1e3,
                       "constant_backward_ms": t_const * 1e3, "one_phase_backward_ms": t_one * 1e3,
                       "four_phase_backward_ms": t_four * 1e3, "one_phase_over_constant": t_one / t_const,
                       "four_phase_over_constant": t_four / t_const,
                       "one_phase_is_constant_bits": bool(all(torch.equal(x.reshape(y.shape), y) for x, y in zip(b, a))),
                       "finite": bool(all(torch.isfinite(g).all() for g in c4)),
                       "deterministic": bool(all(torch.equal(x, y) for x, y in zip(c4, c4_again)))})
    print(line, flush=True)
    if opt.out:
        with open(opt.out, "a") as f:
            f.write(line + "\n")
