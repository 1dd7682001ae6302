#!/usr/bin/env python3
"""Monte-Carlo SIR labels: the per-edge call (gnode_sir_mc_philox_edges) against the scalar call, HIP events around each
call, 10 000 trajectories x 20 steps at wiki-vote size and fb-social size, beta 0.3 / gamma 0.2 and beta 0.05 / gamma 0.1;
warm-up, then 10 calls, median.

    tools/bench_sir_edges.py [--root DIR] [--mode scalar|edges|both] [--calls 10] [--tag NAME]

--root: the tree whose package (and built library) is measured -- another checkout of this repository, e.g. the parent
commit (--mode scalar there: it has no per-edge call), for the before / after of the scalar call; run the two alternately,
one process each.  --mode edges passes one constant on every CSR entry, so the launch draws the scalar call's coins and
returns its counts (checked).  The per-edge time includes the host-side validation of the nnz weights and the staging of
8 * (nnz + n) bytes of thresholds.  Prints one JSON line per (case, rates, mode)."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--mode", default="both", choices=["scalar", "edges", "both"])
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--tag", default="")
args = ap.parse_args()
for p in (os.path.join(args.root, "gn-ode-sir_amd"), os.path.join(args.root, "oracle")):
    sys.path.insert(0, p)

import numpy as np
import torch

import gnode_oracle as O
from gnode import ode_nn
from gnode.graph import DeviceGraph
from gnode.ode_nn import sir_counts


def timed(fn, calls):
    """ms of each of `calls` calls, between two HIP events on the current stream."""
    out = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    cases = [("wiki-vote-sized", 7066, 100736), ("fb-social-sized", 1893, 13835)]
    points = [(0.3, 0.2), (0.05, 0.1)]
    sims, T = 10000, 20
    for name, n, m in cases:
        rp, ci, _ = O.er_graph(n, m, seed=0)
        g = DeviceGraph(rp, ci)
        seeds = [1, n // 2]
        for beta, gamma in points:
            ref = None
            for mode in (["scalar", "edges"] if args.mode == "both" else [args.mode]):
                b = beta if mode == "scalar" else ode_nn.edge_rates(g, np.full(len(ci), beta))
                run = lambda: sir_counts(g, seeds, b, gamma, sims, T, rng_seed=2)
                for _ in range(2):
                    cnt = run()                                     # warm-up
                torch.cuda.synchronize()
                ms = timed(run, args.calls)
                same = None
                if ref is not None:
                    same = bool(torch.equal(cnt, ref))
                ref = cnt
                print(json.dumps({"tag": args.tag, "case": name, "beta": beta, "gamma": gamma, "mode": mode, "sims": sims, "T": T,
                                  "nnz": int(len(ci)), "ms_median": float(np.median(ms)), "ms_min": min(ms), "ms_max": max(ms),
                                  "counts_equal_scalar": same}), flush=True)


if __name__ == "__main__":
    main()
