#!/usr/bin/env python3
"""Monte-Carlo SIR labels: what the initial-state form (gnode_sir_mc_philox_init) costs, and that the seed-list scalar call
did not pay for it.  HIP events around each call, 10 000 trajectories x 20 steps at wiki-vote size and fb-social size, beta
0.3 / gamma 0.2 and beta 0.05 / gamma 0.1; warm-up, then 10 calls, median.

    tools/bench_sir_init.py --parent DIR [--out profiles/sir_init_bench.jsonl] [--calls 10] [--child-timeout 120]
    tools/bench_sir_init.py [--root DIR] --mode scalar|scan|onehot|mixed [--calls 10] [--tag NAME]

--parent: a built checkout of the parent commit.  The seed-list scalar call is then timed on that tree and on this one
alternately, two runs each and one process per run (parent, this, parent, this), followed by the init call on this tree with
a one-hot seed state (the scalar call's counts on rows t >= 1: the run fails if not) and with the mixed state of the tests
(55 % S, 5 % I, 10 % R, 30 % Dirichlet(4, 1, 1) rows), and by one run each of the seed-list call through the edge scan
(`scan`) on the parent and on this tree.  Every record is written to --out (replacing it), then one `verdict` record per
(case, rates): the scalar call's slowdown -- median of this tree's two runs over the median of the parent's -- against the
larger of 2 % and twice the difference between the two parent runs.  The init call's time includes the host-side validation
of the n rows and the staging of 16 n bytes of thresholds.

--mode: one measurement in this process on the tree --root (default: this one); prints one JSON line per (case, rates)."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=HERE)
ap.add_argument("--parent", default=None)
ap.add_argument("--mode", default=None, choices=["scalar", "scan", "onehot", "mixed"])
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "sir_init_bench.jsonl"))
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--tag", default="")
ap.add_argument("--child-timeout", type=float, default=120.0, help="seconds one measuring process may take (a hang or a fault ends the chain)")
args = ap.parse_args()

CASES = [("wiki-vote-sized", 7066, 100736), ("fb-social-sized", 1893, 13835)]
POINTS = [(0.3, 0.2), (0.05, 0.1)]
SIMS, T = 10000, 20


def measure():
    for p in (os.path.join(args.root, "gn-ode-sir_amd"), os.path.join(args.root, "oracle")):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    import gnode_oracle as O
    from gnode import ode_nn
    from gnode.graph import DeviceGraph

    def timed(fn):
        """ms of each call, between two HIP events on the current stream."""
        out = []
        for _ in range(args.calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b))
        return out

    for name, n, m in CASES:
        rp, ci, _ = O.er_graph(n, m, seed=0)
        g = DeviceGraph(rp, ci)
        seeds = [1, n // 2]
        start, same = seeds, None
        if args.mode == "onehot":
            start = ode_nn.InitialState.from_sets(n, seeds)
        elif args.mode == "mixed":
            rng = np.random.default_rng(11)
            kind = rng.choice(4, size=n, p=[0.55, 0.05, 0.10, 0.30])
            p = np.zeros((n, 3))
            for k in range(3):
                p[kind == k, k] = 1.0
            p[kind == 3] = rng.dirichlet([4, 1, 1], size=n)[kind == 3]
            start = ode_nn.initial_state(p)
        for beta, gamma in POINTS:
            run = lambda: ode_nn.sir_counts(g, start, beta, gamma, SIMS, T, rng_seed=2, edge_scan=args.mode == "scan")
            for _ in range(2):
                cnt = run()                                         # warm-up
            torch.cuda.synchronize()
            ms = timed(run)
            if args.mode == "onehot":
                same = bool(torch.equal(cnt[:, 1:], ode_nn.sir_counts(g, seeds, beta, gamma, SIMS, T, rng_seed=2)[:, 1:]))
                if not same:
                    sys.exit(f"{name}, beta {beta}: the one-hot init call's rows t >= 1 differ from the scalar call's")
            print(json.dumps({"tag": args.tag, "case": name, "beta": beta, "gamma": gamma, "mode": args.mode, "sims": SIMS, "T": T,
                              "n": n, "nnz": int(len(ci)), "ms_median": float(np.median(ms)), "ms_min": min(ms), "ms_max": max(ms),
                              "rows_equal_scalar": same}), flush=True)


def drive():
    import statistics
    runs = [(args.parent, "scalar", "parent-1"), (args.root, "scalar", "this-1"), (args.parent, "scalar", "parent-2"),
            (args.root, "scalar", "this-2"), (args.root, "onehot", "this"), (args.root, "mixed", "this"),
            (args.parent, "scan", "parent"), (args.root, "scan", "this")]
    records = []
    for root, mode, tag in runs:                                    # one fresh process per run: one library per process
        # (a fault ends the chain through check=True, a hang through the time limit)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--mode", mode, "--tag", tag, "--calls",
                              str(args.calls)], check=True, stdout=subprocess.PIPE, text=True, timeout=args.child_timeout).stdout
        for line in out.splitlines():
            if line.startswith("{"):
                records.append(json.loads(line))
                print(line, flush=True)
    for name, _, _ in CASES:
        for beta, gamma in POINTS:
            ms = {r["tag"]: r["ms_median"] for r in records if r["mode"] == "scalar" and (r["case"], r["beta"]) == (name, beta)}
            parent, this = statistics.median([ms["parent-1"], ms["parent-2"]]), statistics.median([ms["this-1"], ms["this-2"]])
            bound = max(0.02, 2.0 * abs(ms["parent-1"] - ms["parent-2"]) / parent)
            records.append({"tag": "verdict", "case": name, "beta": beta, "gamma": gamma, "mode": "scalar", "parent_ms": parent,
                            "this_ms": this, "slowdown": this / parent - 1.0, "bound": bound, "within_bound": this / parent - 1.0 <= bound})
            print(json.dumps(records[-1]), flush=True)
    with open(args.out, "w") as fh:                                 # one run, one file: no older verdicts next to these
        for r in records:
            fh.write(json.dumps(r) + "\n")
    return 0 if all(r["within_bound"] for r in records if r["tag"] == "verdict") else 1


if __name__ == "__main__":
    if args.parent:
        sys.exit(drive())
    if not args.mode:
        ap.error("give --parent DIR (the whole comparison) or --mode (one measurement)")
    measure()
