"""Recorder of tests/golden/sir_model_parent.json: a SHA-256 of every array that the four CPU models of the Monte-Carlo SIR
labels returned at commit 35424da (`sir_philox_nodes`, `sir_philox_edges`, `sir_philox_events`, `sir_philox_init`), for every
call of them under tests/ at that commit -- the GPU modules' `_model(...)` and direct calls and the four
test_sir_*_model.py files.  tests/test_sir_model.py holds the one model of tests/sir_model.py to these digests.

THIS SCRIPT CANNOT RUN LATER: the models and the test modules it imports were deleted by the commit that added it.  It ran in a
checkout of 35424da, from its root, and is kept as the statement of what the digests are.  Each entry: `key` (the call site),
`case` (the key in tests/sir_cases.py CASES, or the "cpu/..." case of tests/test_sir_model.py), `fn`, the arguments by recipe,
and per returned array sha256(dtype, shape, bytes)."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ("gn-ode-sir_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import gnode_oracle as O                                                              # noqa: E402
import test_gpu_sir_edges as GE                                                       # noqa: E402
import test_gpu_sir_init as GI                                                        # noqa: E402
import test_gpu_sir_nodes as GN                                                       # noqa: E402
from sir_edges_model import one_way_path, sir_philox_edges                            # noqa: E402
from sir_events_model import sir_philox_events                                        # noqa: E402
from sir_init_model import mixed_init, one_hot_init, sir_philox_init, tree_init       # noqa: E402
from sir_nodes_model import sir_philox_nodes                                          # noqa: E402

NAMES = {"nodes": ("counts",), "edges": ("counts", "t_inf", "t_rec"), "events": ("t_inf", "t_rec", "curves"),
         "init": ("counts", "t_inf", "t_rec")}
ENTRIES = []


def digest(a):
    return hashlib.sha256(f"{a.dtype}{a.shape}".encode() + np.ascontiguousarray(a).tobytes()).hexdigest()


def rec(key, case, fn, out, names=None, **recipe):
    out = out if isinstance(out, tuple) else (out,)
    ENTRIES.append({"key": key, "case": case, "fn": fn, "args": recipe, "sha256": {k: digest(a) for k, a in zip(names or NAMES[fn], out)}})
    print(key, flush=True)
    return out


def nodes(key, case, n, rp, ci, sd, beta, gamma, sims, T, rs, off=0, **recipe):
    return rec(key, case, "nodes", sir_philox_nodes(n, rp, ci, sd, beta, gamma, sims, T, rs, off), sims=sims, T=T, rng_seed=rs, sim_offset=off, **recipe)


def edges(key, case, n, rp, ci, sd, w, gamma, sims, T, rs, off=0, **recipe):
    return rec(key, case, "edges", sir_philox_edges(n, rp, ci, sd, w, gamma, sims, T, rs, off, return_events=True), sims=sims, T=T, rng_seed=rs, sim_offset=off, **recipe)


def events(key, case, n, rp, ci, sd, beta, gamma, sims, T, rs, off=0, **recipe):
    return rec(key, case, "events", sir_philox_events(n, rp, ci, sd, beta, gamma, sims, T, rs, off), sims=sims, T=T, rng_seed=rs, sim_offset=off, **recipe)


def init(key, case, n, rp, ci, p, w, gamma, sims, T, rs, off=0, ev=True, **recipe):
    return rec(key, case, "init", sir_philox_init(n, rp, ci, p, w, gamma, sims, T, rs, off, return_events=ev), sims=sims, T=T, rng_seed=rs, sim_offset=off, **recipe)


def karate():
    import networkx as nx
    from gnode.ode_nn import _csr_from_edges, _edge_arrays
    return (34, *_csr_from_edges(34, _edge_arrays(nx.karate_club_graph())))


def gpu_modules():
    SH = {s[0]: s for s in GN.SHAPES}
    for kind, n, m, seeds, sims, T in GN.SHAPES:                                       # the heterogeneous cases of each file
        rp, ci = GE._csr(kind, n, m)
        hs = GN._hetero_seeds(kind, rp, seeds)
        beta, gamma, _ = GN._rates(kind, n, hs)
        a = nodes(f"gpu_sir_nodes/hetero/{kind}", f"nodes/{kind}", n, rp, ci, hs, beta, gamma, sims, T, 21, shape=kind, seeds="hetero")
        ms = {"wiki-vote-size": 24}.get(kind, sims)
        e = events(f"gpu_sir_traj/model/{kind}", f"nodes/{kind}" + (f"/{ms}" if ms != sims else ""), n, rp, ci, hs, beta, gamma, ms, T, 21, shape=kind, seeds="hetero")
        w, gamma = GE._rates(kind, n, len(ci), hs)
        edges(f"gpu_sir_edges/hetero/{kind}", f"edges/{kind}", n, rp, ci, hs, w, gamma, sims, T, 21, shape=kind, seeds="hetero")
    for kind, n, m, seeds, sims, T in GI.SHAPES:
        rp, ci = GE._csr(kind, n, m)
        w, gamma = GE._rates(kind, n, len(ci), seeds)
        init(f"gpu_sir_init/mixed/{kind}", f"init/{kind}", n, rp, ci, GI._mixed(kind, n, rp), w, gamma, sims, T, 21, shape=kind + " (init)", start="mixed")
    # n = 100 000
    n, seeds = 100_000, [5, 77, 4242]
    rp, ci = GE._csr("large", n, 300_000)
    beta, gamma, _ = GN._rates("large", n, seeds)
    nodes("gpu_sir_nodes/large", "nodes/large", n, rp, ci, seeds, beta, gamma, 24, 8, 99, shape="large", seeds=seeds)
    events("gpu_sir_traj/large", "nodes/large", n, rp, ci, seeds, beta, gamma, 24, 8, 99, shape="large", seeds=seeds)
    w, gamma = GE._rates("large", n, len(ci), seeds)
    edges("gpu_sir_edges/large", "edges/large", n, rp, ci, seeds, w, gamma, 24, 8, 99, shape="large", seeds=seeds)
    init("gpu_sir_init/large", "init/large", n, rp, ci, GI._mixed("large", n, rp), w, gamma, 24, 8, 99, shape="large", start="mixed")
    # er-small: 40 seeds, the second shard
    _, n, m, seeds, _, _ = SH["er-small"]
    rp, ci = GE._csr("er-small", n, m)
    s40 = list(range(3, 3 + 12 * 40, 12))
    beta, gamma, _ = GN._rates("er-small", n, s40)
    nodes("gpu_sir_nodes/seeds40", "nodes/seeds40", n, rp, ci, s40, beta, gamma, 50, 8, 31, shape="er-small", seeds="40 seeds")
    w, gamma = GE._rates("er-small", n, len(ci), s40)
    edges("gpu_sir_edges/seeds40", "edges/seeds40", n, rp, ci, s40, w, gamma, 50, 8, 31, shape="er-small", seeds="40 seeds")
    beta, gamma, _ = GN._rates("er-small", n, seeds)
    nodes("gpu_sir_nodes/shard", "nodes/shard", n, rp, ci, seeds, beta, gamma, 40, 12, 5, 600, shape="er-small", seeds=seeds)
    w, gamma = GE._rates("er-small", n, len(ci), seeds)
    edges("gpu_sir_edges/shard", "edges/shard", n, rp, ci, seeds, w, gamma, 40, 12, 5, 600, shape="er-small", seeds=seeds)
    # isolated from one seed (early extinction)
    _, n, m, seeds, sims, T = SH["isolated"]
    rp, ci = GE._csr("isolated", n, m)
    beta, gamma, _ = GN._rates("isolated", n, seeds)
    events("gpu_sir_traj/isolated-1", "nodes/isolated-1", n, rp, ci, seeds, beta, gamma, sims, T, 21, shape="isolated", seeds=seeds)
    # er300: extreme thresholds, 5 000 trajectories, the connected component
    n = 300
    rp, ci, _ = O.er_graph(n, 600, seed=300)
    depth = GN._bfs_depth(rp, ci, 11, n)
    T = int(depth.max()) + 2
    for name, b, g in (("ones", np.ones(n), np.zeros(n)), ("zeros", np.zeros(n), np.full(n, 0.3)), ("almost", np.full(n, 1.0 - 2.0 ** -33), np.full(n, 0.3))):
        nodes(f"gpu_sir_nodes/{name}", f"nodes/{name}", n, rp, ci, [11], b, g, 32, T, 3, shape="er300", seeds=[11])
    rng = np.random.default_rng(300)
    beta, gamma = rng.uniform(0.05, 0.6, n), rng.uniform(0.05, 0.6, n)
    events("gpu_sir_traj/many", "nodes/many", n, rp, ci, [11, 200], beta, gamma, 5000, 8, 13, shape="er300", seeds=[11, 200])
    keep = np.flatnonzero(depth >= 0)
    new_id = np.full(300, -1)
    new_id[keep] = np.arange(keep.size)
    nc = int(keep.size)
    rpc = np.concatenate([[0], np.cumsum(np.diff(rp)[keep])]).astype(np.int32)
    cic = np.concatenate([new_id[ci[rp[u]:rp[u + 1]]] for u in keep]).astype(np.int32)
    seed = int(new_id[11])
    gamma = np.random.default_rng(9).uniform(0.05, 0.6, nc)
    gamma[seed] = 0.0
    events("gpu_sir_traj/everybody", "nodes/everybody", nc, rpc, cic, [seed], np.ones(nc), gamma, 32, int(GN._bfs_depth(rpc, cic, seed, nc).max()) + 8, 4,
           shape="er300 component of 11", seeds=[seed])
    # karate: the sir_torch surfaces
    n, rp, ci = karate()
    rng = np.random.default_rng(34)
    beta, gamma = rng.uniform(0.05, 0.6, n), rng.uniform(0.05, 0.6, n)
    beta[[4, 20]], beta[8], gamma[12], gamma[30] = 0.0, 1.0, 0.0, 1.0
    nodes("gpu_sir_nodes/karate", "nodes/karate", n, rp, ci, [0, 33], beta, gamma, 300, 12, 77, shape="karate", seeds=[0, 33])
    rng = np.random.default_rng(34)
    w, gamma = rng.uniform(0.05, 0.9, len(ci)), rng.uniform(0.05, 0.6, n)
    w[rng.permutation(len(ci))[:30]] = 0.0
    edges("gpu_sir_edges/karate", "edges/karate", n, rp, ci, [0, 33], w, gamma, 300, 12, 77, shape="karate", seeds=[0, 33])
    p, _ = mixed_init(n, 34)
    init("gpu_sir_init/karate", "init/karate", n, rp, ci, p, 0.3, np.random.default_rng(35).uniform(0.05, 0.6, n), 300, 12, 77, shape="karate", start="mixed_init(34, 34)")
    # the init file's er-small (n = 503) cases
    n = 503
    rp, ci = GE._csr("er-small", n, 2500)
    p = GI._mixed("er-small", n, rp)
    rng = np.random.default_rng(8)
    beta, gamma = rng.uniform(0.05, 0.6, n), rng.uniform(0.05, 0.6, n)
    for name, gm, w in (("scalar", 0.2, 0.3), ("per-node", gamma, beta[ci]), ("per-node beta only", 0.2, beta[ci])):
        init(f"gpu_sir_init/forms-{name}", f"init/forms-{name}", n, rp, ci, p, w, gm, 100, 10, 33, 4, shape="er-small (init)", start="mixed")
    q = np.zeros((n, 3))
    q[0::3], q[1::3], q[2::3] = (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.6, 0.4)
    init("gpu_sir_init/no-S", "init/no-S", n, rp, ci, q, 0.4, np.random.default_rng(9).uniform(0.05, 0.6, n), 100, 10, 51, shape="er-small (init)", start="I / R / (0, .6, .4)")
    q = np.zeros((n, 3))
    q[0::3], q[1::3], q[2::3] = (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.7, 0.0, 0.3)
    init("gpu_sir_init/no-I", "init/no-I", n, rp, ci, q, 0.4, 0.2, 100, 10, 52, shape="er-small (init)", start="S / R / (.7, 0, .3)")
    init("gpu_sir_init/T1", "init/T1", n, rp, ci, p, 0.3, 0.2, 100, 1, 53, shape="er-small (init)", start="mixed")
    w, gamma = GE._rates("er-small", n, len(ci), [3, 499])
    init("gpu_sir_init/shard", "init/shard", n, rp, ci, p, w, gamma, 40, 12, 5, 600, shape="er-small (init)", start="mixed")
    # wiki-vote-size with 40 % infected, isolated with per-node rates
    n = 7066
    rp, ci = GE._csr("wiki-vote-size", n, 100736)
    kind = np.random.default_rng(41).choice(3, size=n, p=[0.5, 0.4, 0.1])
    q = np.zeros((n, 3))
    q[kind == 0, 0], q[kind == 1, 1] = 1.0, 1.0
    q[kind == 2] = (0.5, 0.3, 0.2)
    init("gpu_sir_init/many", "init/many", n, rp, ci, q, 0.05, 0.1, 32, 8, 42, shape="wiki-vote-size", start="50 % S, 40 % I, 10 % (.5, .3, .2)")
    n = 300
    rp, ci = GE._csr("isolated", n, 40)
    rng = np.random.default_rng(12)
    beta, gamma = rng.uniform(0.3, 0.9, n), rng.uniform(0.05, 0.6, n)
    init("gpu_sir_init/isolated-nodes", "init/isolated-nodes", n, rp, ci, GI._mixed("isolated", n, rp), beta[ci], gamma, 64, 6, 61, shape="isolated", start="mixed")
    # test_gpu_sir_lds64k.py: the direct call on its n = 33 000 graph
    n = 33000
    rp, ci, _ = O.er_graph(n, 100000, seed=n)
    rng = np.random.default_rng(n)
    beta, w, gamma = rng.uniform(0.2, 0.8, n), rng.uniform(0.05, 0.9, len(ci)), rng.uniform(0.05, 0.6, n)
    w[rng.permutation(len(ci))[:len(ci) // 5]] = 0.0
    w[::17], gamma[::19], gamma[5::23] = 1.0, 0.0, 1.0
    init("gpu_sir_lds64k/scan-state-in-lds", "init/lds64k", n, rp, ci, mixed_init(n, n + 1)[0], w, gamma, 8, 6, 41, 3, shape="lds64k scan-state-in-lds", start="mixed_init(n, n + 1)")


def cpu_model_tests():
    kar = (34, *O.csr_from_edges(34, [(int(a), int(b)) for a, b in __import__("networkx").karate_club_graph().edges()]))
    er200 = (200, *O.er_graph(200, 800, seed=200)[:2])
    const = [(kar, [0, 33], 0.3, 0.2, 40, 12, 0), (er200, [3, 150], 0.45, 0.15, 24, 10, 0), (er200, [3, 150], 0.05, 0.6, 24, 10, 1000), (kar, [5], 1.0, 0.0, 6, 6, 7)]
    for i, ((n, rp, ci), seeds, beta, gamma, sims, T, off) in enumerate(const):
        for form, b, g in (("both", np.full(n, beta), np.full(n, gamma)), ("beta", np.full(n, beta), gamma), ("gamma", beta, np.full(n, gamma))):
            nodes(f"sir_nodes_model/const/{i}/{form}", f"cpu/const/{i}", n, rp, ci, seeds, b, g, sims, T, 0xABCDEF0123, off, seeds=seeds, rates=[beta, gamma])
        for form, g in (("scalar", gamma), ("array", np.full(n, gamma))):
            rec(f"sir_edges_model/const/{i}/gamma-{form}", f"cpu/const/{i}", "edges",
                sir_philox_edges(n, rp, ci, seeds, np.full(len(ci), beta), g, sims, T, rng_seed=0xABCDEF0123, sim_offset=off),
                seeds=seeds, rates=[beta, gamma], sims=sims, T=T, rng_seed=0xABCDEF0123, sim_offset=off)
    n, rp, ci = er200
    rng = np.random.default_rng(7)
    beta, gamma = rng.uniform(0.2, 0.7, n), rng.uniform(0.1, 0.5, n)
    pos = rng.permutation(np.setdiff1d(np.arange(n), [3, 150]))
    beta[pos[:20]], gamma[pos[20:40]], gamma[pos[40:60]] = 0.0, 1.0, 0.0
    nodes("sir_nodes_model/behave", "cpu/behave", n, rp, ci, [3, 150], beta, gamma, 30, 14, 99, seeds=[3, 150])
    for name, (n, rp, ci) in (("karate", kar), ("er200", er200)):
        rng = np.random.default_rng(17)
        beta, gamma = rng.uniform(0.05, 0.7, n), rng.uniform(0.05, 0.5, n)
        beta[rng.permutation(n)[:n // 8]] = 0.0
        src = np.repeat(np.arange(n), np.diff(rp))
        nodes(f"sir_edges_model/target/{name}/nodes", f"cpu/target/{name}", n, rp, ci, [1, n - 2], beta, gamma, 20, 10, 41, 3, seeds=[1, n - 2])
        rec(f"sir_edges_model/target/{name}/edges", f"cpu/target/{name}", "edges", sir_philox_edges(n, rp, ci, [1, n - 2], beta[ci], gamma, 20, 10, rng_seed=41, sim_offset=3),
            seeds=[1, n - 2], sims=20, T=10, rng_seed=41, sim_offset=3)
        rec(f"sir_edges_model/target/{name}/source", f"cpu/target-src/{name}", "edges", sir_philox_edges(n, rp, ci, [1, n - 2], beta[src], gamma, 20, 10, rng_seed=41, sim_offset=3),
            seeds=[1, n - 2], sims=20, T=10, rng_seed=41, sim_offset=3)
    n, rp, ci, w = one_way_path(12)
    edges("sir_edges_model/path12", "cpu/path12", n, rp, ci, [5], w, 0.0, 7, 10, 9, seeds=[5])
    from gnode.ode_nn import _csr_from_edges, _edge_arrays
    kar2 = (34, *_csr_from_edges(34, _edge_arrays(__import__("networkx").karate_club_graph())))
    for name, (n, rp, ci), seeds, sims, T, rs, off in (("karate", kar2, [0, 33], 40, 12, 77, 9), ("er200", er200, [3, 150, 3], 24, 10, 5, 1000)):
        rng = np.random.default_rng(n)
        beta, gamma = rng.uniform(0.05, 0.6, n), rng.uniform(0.05, 0.6, n)
        beta[5], beta[6], gamma[7], gamma[8] = 0.0, 1.0, 0.0, 1.0
        events(f"sir_events_model/{name}/scalar", f"cpu/events/{name}/scalar", n, rp, ci, seeds, 0.3, 0.2, sims, T, rs, off, seeds=seeds)
        events(f"sir_events_model/{name}/arrays", f"cpu/events/{name}/arrays", n, rp, ci, seeds, beta, gamma, sims, T, rs, off, seeds=seeds)
        nodes(f"sir_events_model/{name}/arrays/nodes", f"cpu/events/{name}/arrays", n, rp, ci, seeds, beta, gamma, sims, T, rs, off, seeds=seeds)
        singles = np.stack([sir_philox_nodes(n, rp, ci, seeds, beta, gamma, 1, T, rs, sim_offset=s) for s in range(off, off + sims)])
        rec(f"sir_events_model/{name}/arrays/singles", f"cpu/events/{name}/arrays", "nodes", singles, names=("singles",), seeds=seeds, sims="1, once per trajectory", T=T, rng_seed=rs, sim_offset=off)
    n, seeds = 203, [3, 77, 202]
    rp, ci, _ = O.er_graph(n, 700, seed=4)
    p = one_hot_init(n, seeds)
    init("sir_init_model/onehot/scalar", "cpu/onehot/scalar", n, rp, ci, p, 0.3, 0.2, 40, 10, 17, 3, ev=False, start="one-hot")
    rng = np.random.default_rng(6)
    w, gamma = rng.uniform(0.05, 0.9, len(ci)), rng.uniform(0.05, 0.6, n)
    w[rng.permutation(len(ci))[:len(ci) // 5]] = 0.0
    a = edges("sir_init_model/onehot/edges", "cpu/onehot/seeds", n, rp, ci, seeds, w, gamma, 40, 10, 18, 2, seeds=seeds)
    b = init("sir_init_model/onehot/init", "cpu/onehot/p", n, rp, ci, p, w, gamma, 40, 10, 18, 2, start="one-hot")
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    n, rp, ci, w, gamma = GE.tree_case()
    init("sir_init_model/tree", "cpu/tree", n, rp, ci, tree_init(), w, gamma, 5000, 12, 1234, ev=False, start="tree_init()")


if __name__ == "__main__":
    gpu_modules()
    cpu_model_tests()
    assert len({e["key"] for e in ENTRIES}) == len(ENTRIES)
    with open(os.path.join(ROOT, "tests", "golden", "sir_model_parent.json"), "w") as f:
        json.dump({"parent": "35424da", "entries": ENTRIES}, f, indent=1)
        f.write("\n")
