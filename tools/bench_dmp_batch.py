#!/usr/bin/env python3
"""The DMP baseline for 16 test samples on one graph: 16 solo `DMP_SIR(...).run(...)` calls (one graph handle
and 2 (maxTime - 1) launches each) against one `dmp_batch` of the same 16 samples.  Both sides include building the graph
handle and copying the result to the host.  One JSON line per graph; no threshold.

    --lib PATH   load this build of libgnode_hip.so instead of the package's, e.g. one compiled with
                 -DGN_DMP_BATCH_GENERAL_ONLY (GNODE_EXTRA_FLAGS of gnode.build), which serves every size with the general
                 form: that is how the one-workgroup form is measured against it.  The line's "lib" says which one ran."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gn-ode-sir_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np, scipy.sparse as sp, torch
import gnode_oracle as O
from gnode import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None)
opt = ap.parse_args()
if opt.lib:
    _lib.LIB_PATH = os.path.abspath(opt.lib)
from gnode.dmp import DMP_SIR, dmp_batch
from gnode.graph import DeviceGraph

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


for name, n, m in (("karate-size", 34, 78), ("er150-size", 150, 700), ("fb-social-size", 4039, 88234)):
    rp, ci, _ = O.er_graph(n, m, seed=1)
    A = sp.csr_matrix((np.ones(len(ci)), ci, rp), shape=(n, n))
    rng = np.random.default_rng(2)
    starts = [sorted(int(s) for s in rng.choice(n, size=2, replace=False)) for _ in range(SAMPLES)]
    scale, gamma = 0.5 / max(1.0, len(ci) / n), 0.3
    g = DeviceGraph(rp, ci)                                  # (kept: the handle dies with it)
    lds = int(_lib.load().gnode_dmp_batch_lds_bytes(g.handle))
    del g

    def solo():
        return [DMP_SIR(A * scale, [gamma] * n).run(s, T).cpu().numpy() for s in starts]

    def batch():
        return dmp_batch(A, starts, gamma, T, scale=[scale] * SAMPLES).cpu().numpy()

    t_solo, t_batch = timed(solo), timed(batch)
    got, want = batch(), solo()
    print(json.dumps({"case": name, "n": n, "nnz": int(len(ci)), "T": T, "samples": SAMPLES, "lib": os.path.basename(opt.lib) if opt.lib else "package",
                      "one_workgroup_lds_bytes": lds, "solo_16_calls_ms": t_solo * 1e3, "batch_1_call_ms": t_batch * 1e3,
                      "bit_equal": bool(all(np.array_equal(got[b], want[b]) for b in range(SAMPLES)))}), flush=True)
