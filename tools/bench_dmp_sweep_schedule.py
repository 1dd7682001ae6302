#!/usr/bin/env python3
"""Source scores and outbreak sizes under a rate schedule: what the scheduled sweeps cost next to the constant ones.  HIP events
around each call and a synchronise; after a warm-up the variants ALTERNATE inside every round, so drift hits them alike;
median, min and max over the rounds.

    tools/bench_dmp_sweep_schedule.py [--root DIR] [--what all|constant] [--rounds 7] [--tag NAME]

At karate size (34 nodes / 156 entries, one workgroup per candidate) and at fb-social size (1 893 nodes / 27 670 entries, the
general form), every node a candidate, T = 30, 16 rows of codes -1 .. 4:
  `events`, `outbreak`              source_scores_events, outbreak_sizes(action="immunise"): the constant entries
  `events-sched-1`, `outbreak-sched-1`   source_scores_schedule, outbreak_sizes_schedule with one phase and shift 0; their
                                    tables are compared with the constant ones (they must be equal bit for bit)
  `events-sched-3`, `outbreak-sched-3`   the same under three phases (the weights scaled 1, 0.25, 0.5; gamma 1, 2, 1 times)
  `observed_at`, `separate`         8 candidates: source_scores_schedule(observed_at=T + 5) against the 8 * T separate
                                    shift-0 calls, one per candidate and start, whose diagonal it is (compared bit for bit)
--root names the tree whose package and built library are measured: with another checkout of this repository that has no
scheduled sweep, e.g. the parent commit, only the constant entries run -- the same code in both trees, so the difference
between the two is the spread of the measurement.  Run the two trees alternately, one process each.  At karate size a call is
a few launches and the host's share dominates, so what else a process runs between two calls shows: --what constant runs the
constant entries alone in this tree too, which is the like-for-like comparison with the parent's.
Prints one JSON line per (case, variant)."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--what", default="all", choices=["all", "constant"])
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--tag", default="")
args = ap.parse_args()
for p in (os.path.join(args.root, "gn-ode-sir_amd"), os.path.join(args.root, "oracle")):
    sys.path.insert(0, p)

import numpy as np
import scipy.sparse as sp
import torch

import gnode_oracle as O
from gnode import dmp as D
from gnode import ode_nn

HAS_SWEEP_SCHEDULE = hasattr(D, "source_scores_schedule") and args.what == "all"
T, R = 30, 16
assert torch.cuda.is_available(), "this measurement needs the GPU"


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


def report(case, times, last, equal_to, **more):
    for name, ms in times.items():
        base = equal_to.get(name)
        same = {} if base is None else {"equals_" + base: bool(torch.equal(last[name], last[base]))}
        print(json.dumps({"tag": args.tag, "case": case, "variant": name, "rounds": len(ms), "ms_median": float(np.median(ms)),
                          "ms_min": min(ms), "ms_max": max(ms), **same, **more}), flush=True)


def main():
    for case, n, m in (("karate-size", 34, 78), ("fb-social-size", 1893, 13835)):
        rp, ci, _ = O.er_graph(n, m, seed=1)
        nnz = len(ci)
        G = D.DmpGraph(sp.csr_matrix((np.full(nnz, 0.5 / max(1.0, nnz / n)), ci, rp), shape=(n, n)))
        rng = np.random.default_rng(3)
        gam = rng.uniform(0.1, 0.5, n)
        rows = rng.choice(np.arange(-1, 5), size=(R, n)).astype(np.int8)
        cands = np.arange(n)
        base = ode_nn.InitialState.from_sets(n, rng.choice(n, size=max(1, n // 20), replace=False))
        lib, handle = D._lib.load(), G.graph.handle
        variants = {"events": lambda: D.source_scores_events(G, rows, gam, T, candidates=cands),
                    "outbreak": lambda: D.outbreak_sizes(G, gam, T, candidates=cands, action="immunise", start=base)}
        equal_to = {}
        if HAS_SWEEP_SCHEDULE:
            steps = np.asarray([0] + [0] * 10 + [1] * 10 + [2] * (T + 6 - 21))            # calendar steps 1 .. T + 5
            scale3, gam3 = ode_nn.rate_schedule([1.0, 0.25, 0.5], steps=steps), ode_nn.rate_schedule([gam, np.minimum(2 * gam, 1.0), gam], steps=steps)
            few, Dcal = cands[:: max(1, n // 8)][:8], T + 5

            def separate():
                padded = np.concatenate([steps[:Dcal + 1], np.full(T - 1, steps[Dcal])])
                out = torch.empty((R, len(few), T), dtype=torch.float64, device="cuda")
                for i, c in enumerate(few):
                    for tau in range(T):
                        row = padded[Dcal - tau:Dcal - tau + T]
                        one = D.source_scores_schedule(G, rows, ode_nn.rate_schedule(gam3.values, steps=row), T, candidates=[c],
                                                       scale=ode_nn.rate_schedule(scale3.values, steps=row))
                        out[:, i, tau] = one[:, 0, tau]
                return out
            variants.update({
                "events-sched-1": lambda: D.source_scores_schedule(G, rows, gam, T, candidates=cands),
                "outbreak-sched-1": lambda: D.outbreak_sizes_schedule(G, gam, T, candidates=cands, action="immunise", start=base),
                "events-sched-3": lambda: D.source_scores_schedule(G, rows, gam3, T, candidates=cands, scale=scale3),
                "outbreak-sched-3": lambda: D.outbreak_sizes_schedule(G, gam3, T, candidates=cands, action="immunise", start=base, scale=scale3),
                "observed_at": lambda: D.source_scores_schedule(G, rows, gam3, T, observed_at=Dcal, candidates=few, scale=scale3),
                "separate": separate})
            equal_to = {"events-sched-1": "events", "outbreak-sched-1": "outbreak", "observed_at": "separate"}
        times, last = alternate(variants, args.rounds)
        report(case, times, last, equal_to, n=n, nnz=int(nnz), T=T, R=R, candidates=int(n),
               one_workgroup=int(lib.gnode_dmp_outbreak_lds_bytes(handle)) <= 160 * 1024)


if __name__ == "__main__":
    main()
