#!/usr/bin/env python3
"""Monte-Carlo SIR labels: the price of the per-trajectory outputs (gnode_sir_mc_philox_traj) against the scalar call, HIP
events around each call, 10 000 trajectories x 20 steps at wiki-vote size and fb-social size, beta 0.3 / 0.05; warm-up,
then 10 calls.

    tools/bench_sir_traj.py [--root DIR] [--modes scalar,curves,events,both] [--calls 10] [--tag NAME]

--root: the tree whose package (and built library) is measured -- another checkout of this repository, e.g. the parent
commit, which knows --modes scalar only, for the before / after of the scalar call (run the two alternately, one process
each).  scalar: `sir_counts`.  curves / events / both: `sir_trajectories` with that output and no counts; the time
includes the allocation of the outputs (cached by torch after the warm-up) and the -1 fill of the events.  Each
trajectory mode is checked once against the scalar call's counts (events -> counts, curves -> node sums).  Prints one
JSON line per (case, rates, mode)."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--modes", default="scalar,curves,events,both")
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
            for mode in args.modes.split(","):
                if mode == "scalar":
                    run = lambda: ode_nn.sir_counts(g, seeds, beta, gamma, sims, T, rng_seed=2)
                else:
                    run = lambda: ode_nn.sir_trajectories(g, seeds, beta, gamma, sims, T, rng_seed=2, events=mode != "curves",
                                                          curves=mode != "events")
                for _ in range(2):
                    out = run()                                     # warm-up
                torch.cuda.synchronize()
                same = None
                if mode == "scalar":
                    ref = out
                elif ref is not None:                               # (after the timing of `scalar`, before this mode's)
                    sums = ref.sum(dim=2).t()[1:]                   # [T - 1, 3]: node sums of the counts = sums of the curves
                    same = True
                    if out.curves is not None:
                        same = same and bool(torch.equal(out.curves[:, 1:].sum(dim=0), sums))
                    if out.t_inf is not None:
                        same = same and bool(torch.equal(ode_nn.sir_counts_from_events(out.t_inf, out.t_rec, T), ref))
                del out
                ms = timed(run, args.calls)
                print(json.dumps({"tag": args.tag, "case": name, "beta": beta, "gamma": gamma, "mode": mode, "sims": sims, "T": T,
                                  "ms_median": float(np.median(ms)), "ms_min": min(ms), "ms_max": max(ms),
                                  "equals_scalar_counts": same}), flush=True)


if __name__ == "__main__":
    main()
