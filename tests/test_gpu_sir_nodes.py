"""GPU: Monte-Carlo SIR labels with per-node infection and recovery rates (gnode_sir_mc_philox_nodes through sir_counts /
sir_torch).  Every comparison is np.array_equal on uint32 counts: against the scalar call where the arrays are constant
(the coins do not move), against the CPU model of tests/sir_nodes_model.py (held to the oracle by
tests/test_sir_nodes_model.py) where they are not."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the shapes of test_gpu_parity.py::test_sir_frontier_equals_edge_scan
SHAPES = [
    ("er-small", 500, 2500, [3, 499], 200, 15),                 # lists in LDS (uint16 ids)
    ("wiki-vote-size", 7066, 100736, [1, 3533], 96, 20),        # lists in LDS, three workgroups per CU
    ("hubs", 3000, 40000, [0, 1, 2999], 64, 12),                # rows longer than 512 edges: walked by the whole workgroup
    ("global-lists", 12000, 60000, [5, 6, 5, 11999], 48, 10),   # lists in the workspace (int32 ids); a duplicated seed
    ("isolated", 300, 40, [7], 64, 6),                          # mostly isolated nodes: the frontier dies out
]
# seeds of the rate draw, one per kind.  `isolated` is 108 because with 105 no beta = 1 node lies next to an infected one
# (check (3) of the heterogeneous test is on the CPU model's output: a seed that fails it is changed, not the check)
RATE_SEED = {"er-small": 101, "wiki-vote-size": 102, "hubs": 103, "global-lists": 104, "isolated": 108, "large": 106}


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gnode import _lib
    _lib.load()                       # fails loudly if libgnode_hip.so is missing
    return torch.device("cuda:0")


_GRAPHS: dict = {}


def _graph(kind, n, m):
    """(rowptr, col, DeviceGraph), built once per module."""
    if kind not in _GRAPHS:
        import gnode_oracle as O
        from gnode.graph import DeviceGraph
        if kind == "hubs":
            rp, ci, _ = O.chung_lu_graph(n, m, exponent=0.95, seed=3)
            assert int(np.max(np.diff(rp))) > 512
        elif kind == "large":
            rp, ci, _ = O.er_graph(n, m, seed=8)
        else:
            rp, ci, _ = O.er_graph(n, m, seed=n)
        _GRAPHS[kind] = (rp, ci, DeviceGraph(rp, ci))
    return _GRAPHS[kind]


def _rates(kind, n, seeds):
    """beta_v, gamma_u ~ U(0.05, 0.6), then at fixed pseudo-random positions 10 % of the nodes beta = 0, 5 % beta = 1,
    5 % gamma = 0, 5 % gamma = 1 (disjoint sets; the seeds keep their drawn rates).  Returns (beta, gamma, sets)."""
    rng = np.random.default_rng(RATE_SEED[kind])
    beta, gamma = rng.uniform(0.05, 0.6, n), rng.uniform(0.05, 0.6, n)
    pos = rng.permutation(np.setdiff1d(np.arange(n), seeds))
    k10, k5 = n // 10, n // 20
    sets = {"b0": pos[:k10], "b1": pos[k10:k10 + k5], "g0": pos[k10 + k5:k10 + 2 * k5], "g1": pos[k10 + 2 * k5:k10 + 3 * k5]}
    beta[sets["b0"]], beta[sets["b1"]], gamma[sets["g0"]], gamma[sets["g1"]] = 0.0, 1.0, 0.0, 1.0
    return beta, gamma, sets


_MODEL: dict = {}


def _model(key, n, rp, ci, seeds, beta, gamma, sims, T, rng_seed, sim_offset=0):
    """The CPU model's counts, computed once per case and shared (never modified)."""
    if key not in _MODEL:
        from sir_nodes_model import sir_philox_nodes
        c = sir_philox_nodes(n, rp, ci, seeds, beta, gamma, sims, T, rng_seed, sim_offset)
        c.setflags(write=False)
        _MODEL[key] = c
    return _MODEL[key]


def _u32(t):
    return t.cpu().numpy().astype(np.uint32)


@pytest.mark.parametrize("kind,n,m,seeds,sims,T", SHAPES, ids=[s[0] for s in SHAPES])
def test_constant_arrays_equal_scalar_call(kind, n, m, seeds, sims, T, dev):
    """The feature's main invariant: arrays that hold one constant each return the scalar call's counts, bit for bit --
    both arrays, array beta with scalar gamma, and the reverse; numpy, list and torch (GPU) inputs."""
    import torch
    from gnode.ode_nn import sir_counts
    rp, ci, g = _graph(kind, n, m)
    for beta, gamma, rs in ((0.45, 0.15, 11), (0.05, 0.6, 12)):
        want = _u32(sir_counts(g, seeds, beta, gamma, sims, T, rng_seed=rs, sim_offset=5))
        assert want[1, 1:].any()
        forms = (("both", np.full(n, beta), np.full(n, gamma)), ("beta", [beta] * n, gamma),
                 ("gamma", beta, torch.full((n,), gamma, dtype=torch.float64, device=dev)))
        for what, b, gm in forms:
            got = _u32(sir_counts(g, seeds, b, gm, sims, T, rng_seed=rs, sim_offset=5))
            assert np.array_equal(got, want), f"{kind}: per-node call with constant {what} != scalar call (beta={beta})"
        got = _u32(sir_counts(g, seeds, np.full(n, beta), np.full(n, gamma), sims, T, rng_seed=rs, sim_offset=5, edge_scan=True))
        assert np.array_equal(got, want), f"{kind}: per-node edge scan with constant arrays != scalar call (beta={beta})"


def _hetero_seeds(kind, rp, seeds):
    """The seed set of the heterogeneous case.  `isolated` (40 edges on 300 nodes: components of two or three nodes) cannot
    carry an epidemic to a quarter of its connected nodes from one seed, whatever the coins: it is seeded in every third
    connected node as well, which also starts many frontiers that die at once."""
    if kind != "isolated":
        return seeds
    return seeds + np.flatnonzero(np.diff(rp) > 0)[::3].tolist()


@pytest.mark.parametrize("kind,n,m,seeds,sims,T", SHAPES, ids=[s[0] for s in SHAPES])
def test_heterogeneous_rates_equal_cpu_model(kind, n, m, seeds, sims, T, dev):
    """Frontier walk and edge scan with a different beta and gamma on every node, shielded (beta = 0), certain
    (beta = 1), never-recovering and always-recovering nodes among them, against the CPU model.  The model's output is
    first checked for a live epidemic, so that two dead ones cannot pass for agreement."""
    from gnode.ode_nn import sir_counts
    rp, ci, g = _graph(kind, n, m)
    seeds = _hetero_seeds(kind, rp, seeds)
    beta, gamma, sets = _rates(kind, n, seeds)
    want = _model(kind, n, rp, ci, seeds, beta, gamma, sims, T, 21)
    S_last = want[0, -1].astype(np.int64)
    deg = np.diff(rp)
    # (1) of the (node, trajectory) pairs whose node is connected and not shielded, a quarter have left S by the last step
    open_nodes = (deg > 0) & (beta > 0.0)
    left = float((sims - S_last[open_nodes]).sum()) / (sims * int(open_nodes.sum()))
    print(f"{kind}: {left:.3f} of the open (node, trajectory) pairs left S")
    assert left >= 0.25
    # (2) shielded nodes stay in S in every trajectory at every step, and at least one of them had an infected neighbour
    touched = S_last < sims                                   # infected in some trajectory (seeds included)
    exposed = [v for v in sets["b0"] if touched[ci[rp[v]:rp[v + 1]]].any()]
    assert exposed and np.all(want[0, 1:][:, sets["b0"]] == sims)
    # (3) a beta = 1 node and a gamma = 1 node were infected
    assert touched[sets["b1"]].any() and touched[sets["g1"]].any()
    a = _u32(sir_counts(g, seeds, beta, gamma, sims, T, rng_seed=21))
    assert np.array_equal(a, want), f"{kind}: frontier walk != CPU model"
    b = _u32(sir_counts(g, seeds, beta, gamma, sims, T, rng_seed=21, edge_scan=True))
    assert np.array_equal(b, want), f"{kind}: edge scan != CPU model"


def test_large_state_paths(dev):
    """n = 100 000: the scan kernel keeps the trajectory state in memory, the frontier walk its lists (int32 ids)."""
    from gnode.ode_nn import sir_counts
    n, seeds = 100_000, [5, 77, 4242]
    rp, ci, g = _graph("large", n, 300_000)
    beta, gamma, _ = _rates("large", n, seeds)
    want = _model("large", n, rp, ci, seeds, beta, gamma, 24, 8, 99)
    assert (want[0, -1] < 24).sum() > 1000
    assert np.array_equal(_u32(sir_counts(g, seeds, beta, gamma, 24, 8, rng_seed=99)), want)
    assert np.array_equal(_u32(sir_counts(g, seeds, beta, gamma, 24, 8, rng_seed=99, edge_scan=True)), want)


def test_more_than_32_seeds(dev):
    """40 seeds: the list is copied from the host instead of travelling as a kernel argument."""
    from gnode.ode_nn import sir_counts
    n = 500
    rp, ci, g = _graph("er-small", n, 2500)
    seeds = list(range(3, 3 + 12 * 40, 12))
    assert len(seeds) == 40 and max(seeds) < n
    beta, gamma, _ = _rates("er-small", n, seeds)
    want = _model("seeds40", n, rp, ci, seeds, beta, gamma, 50, 8, 31)
    assert np.array_equal(_u32(sir_counts(g, seeds, beta, gamma, 50, 8, rng_seed=31)), want)
    assert np.array_equal(_u32(sir_counts(g, seeds, beta, gamma, 50, 8, rng_seed=31, edge_scan=True)), want)


def test_sharded_equals_whole(dev):
    """Two shards of the sims range accumulated into one array equal one call, with heterogeneous rates."""
    import torch
    from gnode.ode_nn import sir_counts
    n, seeds = 500, [3, 499]
    rp, ci, g = _graph("er-small", n, 2500)
    beta, gamma, _ = _rates("er-small", n, seeds)
    whole = sir_counts(g, seeds, beta, gamma, 1000, 12, rng_seed=5)
    acc = sir_counts(g, seeds, beta, gamma, 600, 12, rng_seed=5, sim_offset=0)
    acc = sir_counts(g, seeds, beta, gamma, 400, 12, rng_seed=5, sim_offset=600, counts=acc)
    assert torch.equal(whole, acc)
    assert whole[2, -1].sum().item() > 0
    # the second shard alone is the model's trajectories 600..999
    part = _u32(sir_counts(g, seeds, beta, gamma, 40, 12, rng_seed=5, sim_offset=600))
    assert np.array_equal(part, _model("shard", n, rp, ci, seeds, beta, gamma, 40, 12, 5, 600))


def _bfs_depth(rp, ci, root, n):
    depth = np.full(n, -1)
    depth[root] = 0
    frontier = [root]
    while frontier:
        nxt = []
        for u in frontier:
            for v in ci[rp[u]:rp[u + 1]]:
                if depth[v] < 0:
                    depth[v] = depth[u] + 1
                    nxt.append(int(v))
        frontier = nxt
    return depth


def test_extreme_thresholds(dev):
    """p = 1 always fires (its threshold 2^32 does not fit 32 bits), p = 0 never does, and p = 1 - 2^-33, whose threshold
    is 2^32 - 1, is not p = 1: the 64-bit compare of the scalar path."""
    import gnode_oracle as O
    from gnode.graph import DeviceGraph
    from gnode.ode_nn import sir_counts
    n, seed, sims = 300, 11, 32
    rp, ci, _ = O.er_graph(n, 600, seed=300)
    g = DeviceGraph(rp, ci)
    depth = _bfs_depth(rp, ci, seed, n)
    comp, ecc = depth >= 0, int(depth.max())
    assert comp.sum() > 200 and ecc >= 4
    T = ecc + 2
    ones, zeros = np.ones(n), np.zeros(n)
    # beta = 1, gamma = 0: the infection advances one BFS level per step and nobody recovers
    got = _u32(sir_counts(g, [seed], ones, zeros, sims, T, rng_seed=3))
    for t in range(1, T):
        assert np.array_equal(got[1, t], np.where(comp & (depth <= t), sims, 0)), t
    assert np.all(got[1, ecc][comp] == sims) and not got[2].any()
    assert np.array_equal(got, _model("ones", n, rp, ci, [seed], ones, zeros, sims, T, 3))
    assert np.array_equal(_u32(sir_counts(g, [seed], ones, zeros, sims, T, rng_seed=3, edge_scan=True)), got)
    # beta = 0: nothing but the seed ever leaves S
    got0 = _u32(sir_counts(g, [seed], zeros, np.full(n, 0.3), sims, T, rng_seed=3))
    others = np.arange(n) != seed
    assert np.all(got0[0, 1:][:, others] == sims) and np.all(got0[0, 1:, seed] == 0)
    assert np.array_equal(got0, _model("zeros", n, rp, ci, [seed], zeros, np.full(n, 0.3), sims, T, 3))
    # beta = 1 - 2^-33 -> threshold 2^32 - 1: fires unless the coin word is 2^32 - 1
    almost = np.full(n, 1.0 - 2.0 ** -33)
    assert int(O.coin_threshold(almost[0])) == 2 ** 32 - 1 and int(O.coin_threshold(1.0)) == 2 ** 32
    for scan in (False, True):
        gota = _u32(sir_counts(g, [seed], almost, np.full(n, 0.3), sims, T, rng_seed=3, edge_scan=scan))
        assert np.array_equal(gota, _model("almost", n, rp, ci, [seed], almost, np.full(n, 0.3), sims, T, 3))


def test_sir_torch_surface(dev):
    """Arrays through the reference-shaped surface: float64 [1, T, n] counts, rates indexed by node id."""
    import networkx as nx
    from gnode.ode_nn import _csr_from_edges, _edge_arrays, sir_torch
    G = nx.karate_club_graph()
    n, sims, T, seeds = 34, 300, 12, [0, 33]
    rp, ci = _csr_from_edges(n, _edge_arrays(G))
    rng = np.random.default_rng(34)
    beta, gamma = rng.uniform(0.05, 0.6, n), rng.uniform(0.05, 0.6, n)
    beta[[4, 20]], beta[8], gamma[12], gamma[30] = 0.0, 1.0, 0.0, 1.0
    want = _model("karate", n, rp, ci, seeds, beta, gamma, sims, T, 77).astype(np.float64)
    assert want[2, -1].sum() > 0
    S, I, R = sir_torch(G, seeds, beta, gamma.tolist(), sims, T, rng_seed=77)
    assert S.shape == (1, T, n) and S.dtype == np.float64
    assert np.array_equal(S[0], want[0]) and np.array_equal(I[0], want[1]) and np.array_equal(R[0], want[2])
    S1, I1, R1 = sir_torch(G, seeds, beta, gamma, sims, T, rng_seed=77, normalize_t0=True)
    want[:, 0] *= sims
    assert np.array_equal(S1[0], want[0]) and np.array_equal(I1[0], want[1]) and np.array_equal(R1[0], want[2])


def test_scalar_path_untouched_after_per_node_calls(dev):
    """No state leaks through the handle or the workspace: a scalar call after per-node calls still equals the oracle."""
    import oracle_c as OC
    from gnode.ode_nn import sir_counts
    n, seeds = 500, [3, 499]
    rp, ci, g = _graph("er-small", n, 2500)
    beta, gamma, _ = _rates("er-small", n, seeds)
    sir_counts(g, seeds, beta, gamma, 64, 10, rng_seed=9)
    sir_counts(g, seeds, beta, 0.2, 64, 10, rng_seed=9, edge_scan=True)
    for scan in (False, True):
        got = _u32(sir_counts(g, seeds, 0.3, 0.2, 64, 10, rng_seed=9, edge_scan=scan))
        assert np.array_equal(got, OC.sir_philox(n, rp, ci, seeds, 0.3, 0.2, 64, 10, rng_seed=9))
