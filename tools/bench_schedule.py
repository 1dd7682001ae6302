#!/usr/bin/env python3
"""Rates that change over time: what the scheduled entries cost next to the constant ones.  HIP events around each
synchronised call; after a warm-up the variants ALTERNATE inside every round, so drift hits them alike; median, min and max
over the rounds.

    tools/bench_schedule.py [--root DIR] [--what sir|dmp|all] [--rounds 7] [--tag NAME]

sir   10 000 trajectories x 20 steps at wiki-vote size (7 066 nodes / 100 736 entries), one constant weight per entry:
      `edges`       gnode_sir_mc_philox_edges
      `sched-1`     gnode_sir_mc_philox_schedule with one phase
      `sched-4`     the same with four phases that hold equal tables, visited in turn
      The counts of the three are compared (they must be equal).  --root names the tree whose package and built library are
      measured: with another checkout of this repository, e.g. the parent commit, only `edges` runs (it has no scheduled
      entry) -- the same code in both trees, so the difference between the two is the spread of the measurement.  Run the two
      trees alternately, one process each.
dmp   dmp_batch against the scheduled call with one phase, B = 64, T = 20: at hub size (3 001 nodes / 80 000 entries, the
      general form) and on a graph of 300 nodes / 1 800 entries (the one-workgroup form).  Outputs are compared bit for bit.
Prints one JSON line per (case, variant)."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--what", default="all", choices=["sir", "dmp", "all"])
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--tag", default="")
args = ap.parse_args()
for p in (os.path.join(args.root, "gn-ode-sir_amd"), os.path.join(args.root, "oracle")):
    sys.path.insert(0, p)

import numpy as np
import torch

import gnode_oracle as O
from gnode import dmp as D
from gnode import ode_nn
from gnode.graph import DeviceGraph

HAS_SCHEDULE = hasattr(ode_nn, "rate_schedule")


def alternate(variants, rounds):
    """{name: [ms per round]} and {name: last result}: two warm-up rounds, then every variant once per round, in turn."""
    times, last = {k: [] for k in variants}, {}
    for r in range(rounds + 2):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            last[name] = fn()
            b.record()
            b.synchronize()
            if r >= 2:
                times[name].append(a.elapsed_time(b))
    return times, last


def report(case, times, last, base, **more):
    for name, ms in times.items():
        print(json.dumps({"tag": args.tag, "case": case, "variant": name, "rounds": len(ms), "ms_median": float(np.median(ms)),
                          "ms_min": min(ms), "ms_max": max(ms), "equals_" + base: bool(torch.equal(last[name], last[base])), **more}), flush=True)


def sir():
    n, m, sims, T, beta, gamma = 7066, 100736, 10000, 20, 0.3, 0.2
    rp, ci, _ = O.er_graph(n, m, seed=0)
    g = DeviceGraph(rp, ci)
    seeds = [1, n // 2]
    er = ode_nn.edge_rates(g, np.full(len(ci), beta))
    variants = {"edges": lambda: ode_nn.sir_counts(g, seeds, er, gamma, sims, T, rng_seed=2)}
    if HAS_SCHEDULE:
        one = ode_nn.rate_schedule([er], starts=[1])
        four = ode_nn.rate_schedule([er] * 4, steps=np.arange(T) % 4)
        four_g = ode_nn.rate_schedule([gamma] * 4, steps=np.arange(T) % 4)
        variants["sched-1"] = lambda: ode_nn.sir_counts(g, seeds, one, gamma, sims, T, rng_seed=2)
        variants["sched-4"] = lambda: ode_nn.sir_counts(g, seeds, four, four_g, sims, T, rng_seed=2)
    times, last = alternate(variants, args.rounds)
    report("sir/wiki-vote-size", times, last, "edges", sims=sims, T=T, nnz=int(len(ci)))


def dmp():
    import scipy.sparse as sp
    B, T = 64, 20
    hub = O.chung_lu_graph(3001, 40000, seed=2)[:2]
    small = O.er_graph(300, 900, seed=7)[:2]
    for case, (rp, ci) in (("dmp/hub-size", hub), ("dmp/one-workgroup", small)):
        n, nnz = len(rp) - 1, len(ci)
        rng = np.random.default_rng(5)
        s = min(1.0, 5.0 * n / nnz)
        M = sp.csr_matrix((rng.uniform(0.05 * s, 0.4 * s, nnz), ci, rp), shape=(n, n))
        G = D.DmpGraph(M)
        starts = [[int(v)] for v in rng.integers(0, n, B)]
        gam = rng.uniform(0.1, 0.5, n)
        lds = int(D._lib.load().gnode_dmp_batch_lds_bytes(G.graph.handle))
        variants = {"dmp_batch": lambda: D.dmp_batch(G, starts, gam, T)}
        if HAS_SCHEDULE:
            sched = ode_nn.rate_schedule([gam], starts=[1])
            variants["sched-1"] = lambda: D.dmp_batch(G, starts, sched, T)
        times, last = alternate(variants, args.rounds)
        report(case, times, last, "dmp_batch", B=B, T=T, n=n, nnz=nnz, one_workgroup=lds <= 160 * 1024)


if __name__ == "__main__":
    if args.what in ("sir", "all"):
        sir()
    if args.what in ("dmp", "all"):
        dmp()
