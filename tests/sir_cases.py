"""The cases of the Monte-Carlo SIR tests, stated once (a helper, not a test): shapes, graphs, rate and start draws, the
named model cases with their expected arrays, and the liveness checks on those.

Everything here but `dev`, `graph`, `er_of` and `state` is numpy only.  `case(key)` builds the inputs of a named case,
`expected(key)` runs tests/sir_model.py on it, once, and returns read-only arrays.  tests/test_sir_model.py holds every case to
the arrays the four earlier models returned for it (tests/golden/sir_model_parent.json) and runs its liveness checks without a
GPU; the GPU modules reach their expected arrays through the same two functions."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import sir_model as M
from sir_init_model import tree_init

SHAPES = [
    ("er-small", 500, 2500, [3, 499], 200, 15),                 # lists in LDS (uint16 ids)
    ("wiki-vote-size", 7066, 100736, [1, 3533], 96, 20),        # lists in LDS, three workgroups per CU
    ("hubs", 3000, 40000, [0, 1, 2999], 64, 12),                # rows longer than 512 edges: walked by the whole workgroup
    ("global-lists", 12000, 60000, [5, 6, 5, 11999], 48, 10),   # lists in the workspace (int32 ids); a duplicated seed
    ("isolated", 300, 40, [7], 64, 6),                          # mostly isolated nodes: the frontier dies out
]
# the same with n ragged where the generator allows it: the last Philox block of the start's node coins is partial
INIT_SHAPES = [(k, n + {"er-small": 3, "global-lists": 1}.get(k, 0), m, s, sims, T) for k, n, m, s, sims, T in SHAPES]
IDS = [s[0] for s in SHAPES]
SHAPE, INIT_SHAPE = {s[0]: s for s in SHAPES}, {s[0]: s for s in INIT_SHAPES}
LARGE = ("large", 100_000, 300_000, [5, 77, 4242], 24, 8)       # the scan keeps its state in memory, the walk int32 lists
SEEDS40 = list(range(3, 3 + 12 * 40, 12))                       # more seeds than travel as a kernel argument
# seeds of the draws, one per kind.  The liveness checks are on the model's output: a seed that fails them is changed, not
# the check (`isolated` is 108 for the per-node rates because with 105 no beta = 1 node lies next to an infected one)
NODE_RATE_SEED = {"er-small": 101, "wiki-vote-size": 102, "hubs": 103, "global-lists": 104, "isolated": 108, "large": 106}
EDGE_RATE_SEED = {"er-small": 201, "wiki-vote-size": 202, "hubs": 203, "global-lists": 204, "isolated": 205, "large": 206}
INIT_SEED = {"er-small": 301, "wiki-vote-size": 302, "hubs": 303, "global-lists": 304, "isolated": 305, "large": 306}
LDS64K_SCAN, LDS64K_FRONTIER = ("scan-state-in-lds", 33000, 100000, True), ("frontier", 153000, 460000, False)
LDS64K_SIMS, LDS64K_T, LDS64K_RNG = 8, 6, 41


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gnode import _lib
    _lib.load()                       # fails loudly if libgnode_hip.so is missing
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------- graphs
@functools.lru_cache(maxsize=None)
def csr(kind, n, m, seed=None):
    """(rowptr, col) of a shape, read-only, built once per (kind, n, m); an ER graph under seed n unless one is given."""
    import gnode_oracle as O
    if kind == "hubs":
        rp, ci, _ = O.chung_lu_graph(n, m, exponent=0.95, seed=3)
        assert int(np.max(np.diff(rp))) > 512
    else:
        rp, ci, _ = O.er_graph(n, m, seed=(8 if kind == "large" else n) if seed is None else seed)
    return _frozen(rp), _frozen(ci)


@functools.lru_cache(maxsize=None)
def graph(kind, n, m):
    """(rowptr, col, DeviceGraph), built once per (kind, n, m)."""
    from gnode.graph import DeviceGraph
    rp, ci = csr(kind, n, m)
    return rp, ci, DeviceGraph(rp, ci)


def _frozen(a):
    """The array, read-only if it is one: what a cache hands to several tests stays what it was."""
    if isinstance(a, np.ndarray):
        a.setflags(write=False)
    return a


def er200():
    return (200, *csr("er200", 200, 800))


def er300():
    """(300, rowptr, col): the graph of the extreme-rate and many-trajectory tests (`graph("er300", 300, 600)` on the GPU)."""
    return (300, *csr("er300", 300, 600))


def er300_component():
    """(n, rowptr, col, seed): the component of node 11 of `er300`, renumbered (a component keeps whole rows)."""
    _, rp0, ci0 = er300()
    keep = np.flatnonzero(bfs_depth(rp0, ci0, 11, 300) >= 0)
    new_id = np.full(300, -1)
    new_id[keep] = np.arange(keep.size)
    rp = np.concatenate([[0], np.cumsum(np.diff(rp0)[keep])]).astype(np.int32)
    ci = np.concatenate([new_id[ci0[rp0[u]:rp0[u + 1]]] for u in keep]).astype(np.int32)
    assert ci.min() >= 0 and rp[-1] == ci.size
    return int(keep.size), rp, ci, int(new_id[11])


def karate():
    import networkx as nx
    from gnode.ode_nn import _csr_from_edges, _edge_arrays
    G = nx.karate_club_graph()
    return (G, 34, *_csr_from_edges(34, _edge_arrays(G)))


def bfs_depth(rp, ci, root, n):
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


def tree_case():
    """The DMP comparison's inputs: a random recursive tree of 120 nodes, asymmetric weights with closed and certain entries,
    per-node gamma."""
    import gnode_oracle as O
    n = 120
    rng = np.random.default_rng(5)
    edges = [(int(rng.integers(0, i)), i) for i in range(1, n)]
    rp, ci = O.csr_from_edges(n, edges)
    nnz = len(ci)
    assert nnz == 2 * (n - 1)
    rng = np.random.default_rng(7)
    w = rng.uniform(0.3, 0.95, nnz)
    pos = rng.permutation(nnz)
    w[pos[:nnz // 10]], w[pos[nnz // 10:nnz // 10 + nnz // 20]] = 0.0, 1.0
    gamma = rng.uniform(0.05, 0.3, n)
    return n, rp, ci, w, gamma


def dmp_ratio(counts, sims, P):
    """max over the cells of rows t >= 1 of |count / sims - P| / (sqrt(P (1 - P) / sims) + 1 / sims); counts uint32
    [3, T, n], P float64 [T, n, 3]."""
    f = counts[:, 1:].astype(np.float64).transpose(1, 2, 0) / sims
    p = np.clip(P[1:], 0.0, 1.0)
    return float(np.max(np.abs(f - P[1:]) / (np.sqrt(p * (1.0 - p) / sims) + 1.0 / sims)))


class StubGraph:
    """What the Monte-Carlo calls read before they enter the library.  `handle` raises: reaching it means a check came too late."""
    n, nnz = 10, 18
    rowptr = np.concatenate([[0], np.cumsum([1] + [2] * 8 + [1])])
    col = np.asarray([j for i in range(10) for j in (i - 1, i + 1) if 0 <= j < 10])

    @property
    def handle(self):
        raise AssertionError("the library was entered before the rates were checked")


# ------------------------------------------------------------------------------------------------------ rates and starts
def node_rates(kind, n, seeds):
    """beta_v, gamma_u ~ U(0.05, 0.6), then at fixed pseudo-random positions 10 % of the nodes beta = 0, 5 % beta = 1,
    5 % gamma = 0, 5 % gamma = 1 (disjoint sets; the seeds keep their drawn rates).  Returns (beta, gamma, sets)."""
    rng = np.random.default_rng(NODE_RATE_SEED[kind])
    beta, gamma = rng.uniform(0.05, 0.6, n), rng.uniform(0.05, 0.6, n)
    pos = rng.permutation(np.setdiff1d(np.arange(n), seeds))
    k10, k5 = n // 10, n // 20
    sets = {"b0": pos[:k10], "b1": pos[k10:k10 + k5], "g0": pos[k10 + k5:k10 + 2 * k5], "g1": pos[k10 + 2 * k5:k10 + 3 * k5]}
    beta[sets["b0"]], beta[sets["b1"]], gamma[sets["g0"]], gamma[sets["g1"]] = 0.0, 1.0, 0.0, 1.0
    return beta, gamma, sets


def edge_weights(kind, n, nnz, seeds):
    """w ~ U(0.05, 0.9) independently per directed entry (so w[u -> v] != w[v -> u]), then at fixed pseudo-random positions
    20 % of the entries 0 and 5 % of them 1; gamma_u ~ U(0.05, 0.6) with 5 % of the nodes 0 and 5 % 1, as in the per-node
    draw (the seeds keep their drawn gamma).  Returns (w, gamma)."""
    rng = np.random.default_rng(EDGE_RATE_SEED[kind])
    w, gamma = rng.uniform(0.05, 0.9, nnz), rng.uniform(0.05, 0.6, n)
    epos = rng.permutation(nnz)
    w[epos[:nnz // 5]], w[epos[nnz // 5:nnz // 5 + nnz // 20]] = 0.0, 1.0
    npos = rng.permutation(np.setdiff1d(np.arange(n), seeds))
    gamma[npos[:n // 20]], gamma[npos[n // 20:2 * (n // 20)]] = 0.0, 1.0
    return w, gamma


@functools.lru_cache(maxsize=None)
def lds64k_case(kind, n, m):
    """graph, start and rates of an lds64k shape, numpy only: (rowptr, col, seeds, p, beta, w, gamma)"""
    rp, ci = csr(kind, n, m)
    rng = np.random.default_rng(n)
    beta, w, gamma = rng.uniform(0.2, 0.8, n), rng.uniform(0.05, 0.9, len(ci)), rng.uniform(0.05, 0.6, n)
    w[rng.permutation(len(ci))[:len(ci) // 5]] = 0.0                # directed contacts
    w[::17], gamma[::19], gamma[5::23] = 1.0, 0.0, 1.0
    return tuple(_frozen(a) for a in (rp, ci, [7, n // 2, n - 1], M.mixed_init(n, n + 1)[0], beta, w, gamma))


def hetero_seeds(kind, rp, seeds):
    """The seed set of the heterogeneous cases.  `isolated` (40 edges on 300 nodes: components of two or three nodes) cannot
    carry an epidemic to a quarter of its connected nodes from one seed, whatever the coins: it is seeded in every third
    connected node as well, which also starts many frontiers that die at once."""
    if kind != "isolated":
        return seeds
    return seeds + np.flatnonzero(np.diff(rp) > 0)[::3].tolist()


def mixed_start(kind, n, rp):
    """55 % S, 5 % I, 10 % R and 30 % Dirichlet(4, 1, 1) rows under the kind's seed.  `isolated` cannot lose a quarter of its
    susceptible connected nodes from that, whatever the coins: every third connected node starts infected as well."""
    p, _ = M.mixed_init(n, INIT_SEED[kind])
    if kind == "isolated":
        p[np.flatnonzero(np.diff(rp) > 0)[::3]] = (0.0, 1.0, 0.0)
    return p


def u32(t):
    return t.cpu().numpy().astype(np.uint32)


def er_of(g, w):
    from gnode.ode_nn import edge_rates
    return edge_rates(g, w)


def state(p):
    from gnode.ode_nn import initial_state
    return initial_state(p)


# ------------------------------------------------------------------------------------------------------ liveness checks
def live_nodes(c, want):
    """On the model's own output, per-node rates: (1) of the (node, trajectory) pairs whose node is connected and not
    shielded, a quarter have left S by the last step; (2) shielded nodes stay in S in every trajectory at every step, and at
    least one of them had an infected neighbour; (3) a beta = 1 node and a gamma = 1 node were infected."""
    S_last = want.counts[0, -1].astype(np.int64)
    open_nodes = (np.diff(c.rp) > 0) & (c.beta > 0.0)
    left = float((c.sims - S_last[open_nodes]).sum()) / (c.sims * int(open_nodes.sum()))
    print(f"{c.kind}: {left:.3f} of the open (node, trajectory) pairs left S")
    assert left >= 0.25
    touched = S_last < c.sims                                 # infected in some trajectory (seeds included)
    exposed = [v for v in c.sets["b0"] if touched[c.ci[c.rp[v]:c.rp[v + 1]]].any()]
    assert exposed and np.all(want.counts[0, 1:][:, c.sets["b0"]] == c.sims)
    assert touched[c.sets["b1"]].any() and touched[c.sets["g1"]].any()


def live_edges(c, want):
    """On the model's own output, per-edge weights: (1) at least a quarter of the (connected node, trajectory) pairs left S;
    (2) a w = 1 entry fired; (3) some w = 0 entry had an infected source next to a susceptible target in a pre-step state."""
    t_inf, t_rec = want.t_inf, want.t_rec
    connected = np.diff(c.rp) > 0
    left = float((t_inf[:, connected] >= 0).sum()) / (c.sims * int(connected.sum()))
    print(f"{c.kind}: {left:.3f} of the (connected node, trajectory) pairs left S")
    assert left >= 0.25
    src = np.repeat(np.arange(c.n), np.diff(c.rp))
    one, zero = np.flatnonzero(c.w == 1.0), np.flatnonzero(c.w == 0.0)
    tu, tv, ru = t_inf[:, src[one]].astype(np.int32), t_inf[:, c.ci[one]].astype(np.int32), t_rec[:, src[one]].astype(np.int32)
    # u in I and v in S before step t = t_inf[v]: the entry's coin was drawn at t, and a w = 1 coin fires
    fired = (tu >= 0) & (tv > tu) & ((ru < 0) | (ru >= tv))
    assert fired.any(), f"{c.kind}: no w = 1 entry fired"
    tu, tv = t_inf[:, src[zero]].astype(np.int32), t_inf[:, c.ci[zero]].astype(np.int32)
    blocked = (tu >= 0) & (tu + 1 <= c.T - 1) & ((tv < 0) | (tv > tu))
    assert blocked.any(), f"{c.kind}: no w = 0 entry was ever tried"


def live_events(c, want):
    """On the model's own output: the case exercises every kind of entry of the per-trajectory output."""
    t_inf, t_rec, curves = want.t_inf, want.t_rec, want.curves
    assert (t_inf == -1).any(), f"{c.kind}: every node is infected in every trajectory"
    assert ((t_inf >= 0) & (t_rec == -1)).any(), f"{c.kind}: nobody stays infected to the end"
    assert (t_rec >= 0).any(), f"{c.kind}: nobody recovers"
    assert any(not np.array_equal(curves[0], cv) for cv in curves[1:]), f"{c.kind}: all curves are the same"


def live_init(c, want):
    """On the model's own output, drawn start: at least a quarter of the initially susceptible (connected node, trajectory)
    pairs left S."""
    connected = np.diff(c.rp) > 0
    sus, left = (want.t_inf != 0)[:, connected], (want.t_inf > 0)[:, connected]
    print(f"{c.kind}: {left.sum() / sus.sum():.3f} of the initially susceptible (connected node, trajectory) pairs left S")
    assert left.sum() >= 0.25 * sus.sum()


# ------------------------------------------------------------------------------------------------------- the model cases
def _case(kind, n, rp, ci, start, gamma, sims, T, rng_seed, sim_offset=0, beta=None, w=None, live=(), **more):
    """The arguments of one model call.  `start` is a seed list or p [n, 3]; exactly one of beta (scalar or per node) and w
    (per CSR position) is given; `live` are the liveness checks the case has to pass.  Every array of a case is read-only."""
    fields = dict(kind=kind, n=n, rp=rp, ci=ci, start=start, beta=beta, w=w, gamma=gamma, sims=sims, T=T, rng_seed=rng_seed,
                  sim_offset=sim_offset, live=live, **more)
    return SimpleNamespace(**{k: _frozen(v) for k, v in fields.items()})


def _shape_case(form, kind, seeds=None, sims=None, T=None, rng_seed=21, sim_offset=0, hetero=True, live=()):
    """A case on a graph of the shape table: form "nodes" (seed list, per-node rates), "edges" (seed list, per-edge weights)
    or "init" (the kind's mixed start on the ragged shape, the per-edge weights drawn around the shape's seeds)."""
    shape = LARGE if kind == "large" else (INIT_SHAPE if form == "init" else SHAPE)[kind]
    _, n, m, shape_seeds, shape_sims, shape_T = shape
    rp, ci = csr(kind, n, m)
    seeds = shape_seeds if seeds is None else seeds
    seeds = hetero_seeds(kind, rp, seeds) if hetero else seeds
    sims, T = sims or shape_sims, T or shape_T
    if form == "nodes":
        beta, gamma, sets = node_rates(kind, n, seeds)
        return _case(kind, n, rp, ci, seeds, gamma, sims, T, rng_seed, sim_offset, beta=beta, sets=sets, m=m, live=live)
    w, gamma = edge_weights(kind, n, len(ci), shape_seeds if form == "init" else seeds)
    start = mixed_start(kind, n, rp) if form == "init" else seeds
    return _case(kind, n, rp, ci, start, gamma, sims, T, rng_seed, sim_offset, w=w, m=m, live=live)


def _extreme(kind, beta, gamma):
    n, rp, ci = er300()
    depth = bfs_depth(rp, ci, 11, n)
    return _case(kind, n, rp, ci, [11], np.full(n, gamma), 32, int(depth.max()) + 2, 3, beta=np.full(n, beta), depth=depth)


def _many():
    rng = np.random.default_rng(300)
    beta, gamma = rng.uniform(0.05, 0.6, 300), rng.uniform(0.05, 0.6, 300)
    n, rp, ci = er300()
    return _case("er300 x 5000", n, rp, ci, [11, 200], gamma, 5000, 8, 13, beta=beta, live=(live_events,))


def _everybody():
    n, rp, ci, seed = er300_component()
    ecc = int(bfs_depth(rp, ci, seed, n).max())
    gamma = np.random.default_rng(9).uniform(0.05, 0.6, n)
    gamma[seed] = 0.0
    return _case("everybody", n, rp, ci, [seed], gamma, 32, ecc + 8, 4, beta=np.ones(n))


def _karate(form):
    G, n, rp, ci = karate()
    if form == "init":
        p, _ = M.mixed_init(n, 34)
        return _case("karate", n, rp, ci, p, np.random.default_rng(35).uniform(0.05, 0.6, n), 300, 12, 77, beta=0.3, G=G)
    rng = np.random.default_rng(34)
    if form == "nodes":
        beta, gamma = rng.uniform(0.05, 0.6, n), rng.uniform(0.05, 0.6, n)
        beta[[4, 20]], beta[8], gamma[12], gamma[30] = 0.0, 1.0, 0.0, 1.0
        return _case("karate", n, rp, ci, [0, 33], gamma, 300, 12, 77, beta=beta, G=G)
    w, gamma = rng.uniform(0.05, 0.9, len(ci)), rng.uniform(0.05, 0.6, n)
    w[rng.permutation(len(ci))[:30]] = 0.0
    keep = rng.permutation(np.flatnonzero(w != 0.0))                 # a matrix leaves the zeros out and shuffles the rest
    return _case("karate", n, rp, ci, [0, 33], gamma, 300, 12, 77, w=w, G=G, keep=keep)


def _init_er_small(kind, p, gamma, sims, T, rng_seed, sim_offset=0, beta=None, w=None):
    _, n, m, *_ = INIT_SHAPE["er-small"]
    rp, ci = csr("er-small", n, m)
    return _case(kind, n, rp, ci, mixed_start("er-small", n, rp) if p is None else p, gamma, sims, T, rng_seed, sim_offset, beta=beta, w=w)


def _init_forms(name):
    _, n, m, *_ = INIT_SHAPE["er-small"]
    rng = np.random.default_rng(8)
    beta, gamma = rng.uniform(0.05, 0.6, n), rng.uniform(0.05, 0.6, n)
    b, gm = {"scalar": (0.3, 0.2), "per-node": (beta, gamma), "per-node beta only": (beta, 0.2)}[name]
    return _init_er_small("forms-" + name, None, gm, 100, 10, 33, 4, beta=b)


def _thirds(rows):
    p = np.zeros((INIT_SHAPE["er-small"][1], 3))
    p[0::3], p[1::3], p[2::3] = rows
    return p


def _init_many():
    _, n, m, *_ = INIT_SHAPE["wiki-vote-size"]
    rp, ci = csr("wiki-vote-size", n, m)
    kind = np.random.default_rng(41).choice(3, size=n, p=[0.5, 0.4, 0.1])
    p = np.zeros((n, 3))
    p[kind == 0, 0], p[kind == 1, 1] = 1.0, 1.0
    p[kind == 2] = (0.5, 0.3, 0.2)
    assert (kind == 1).sum() > 0.39 * n
    return _case("many", n, rp, ci, p, 0.1, 32, 8, 42, beta=0.05)


def _init_isolated_nodes():
    _, n, m, *_ = INIT_SHAPE["isolated"]
    rp, ci = csr("isolated", n, m)
    rng = np.random.default_rng(12)
    beta, gamma = rng.uniform(0.3, 0.9, n), rng.uniform(0.05, 0.6, n)
    return _case("isolated-nodes", n, rp, ci, mixed_start("isolated", n, rp), gamma, 64, 6, 61, beta=beta)


def _init_lds64k():
    kind, n, m, _ = LDS64K_SCAN
    rp, ci, _, p, _, w, gamma = lds64k_case(kind, n, m)
    return _case(kind, n, rp, ci, p, gamma, LDS64K_SIMS, LDS64K_T, LDS64K_RNG, 3, w=w)


def _small(graph):
    return er200() if graph == "er200" else karate()[1:]


RS = 0xABCDEF0123
CONST = [("karate", [0, 33], 0.3, 0.2, 40, 12, 0), ("er200", [3, 150], 0.45, 0.15, 24, 10, 0),
         ("er200", [3, 150], 0.05, 0.6, 24, 10, 1000),        # sim_offset: other trajectories' coins
         ("karate", [5], 1.0, 0.0, 6, 6, 7)]                  # the two ends of the threshold range
EVENTS = {"karate": ("karate", [0, 33], 40, 12, 77, 9), "er200": ("er200", [3, 150, 3], 24, 10, 5, 1000)}


def _behave():
    n, rp, ci = er200()
    rng = np.random.default_rng(7)
    beta, gamma = rng.uniform(0.2, 0.7, n), rng.uniform(0.1, 0.5, n)
    pos = rng.permutation(np.setdiff1d(np.arange(n), [3, 150]))
    sets = {"b0": pos[:20], "g1": pos[20:40], "g0": pos[40:60]}
    beta[sets["b0"]], gamma[sets["g1"]], gamma[sets["g0"]] = 0.0, 1.0, 0.0
    return _case("behave", n, rp, ci, [3, 150], gamma, 30, 14, 99, beta=beta, sets=sets)


def _target(graph, by_source):
    n, rp, ci = _small(graph)
    rng = np.random.default_rng(17)
    beta, gamma = rng.uniform(0.05, 0.7, n), rng.uniform(0.05, 0.5, n)
    beta[rng.permutation(n)[:n // 8]] = 0.0
    rate = dict(w=beta[np.repeat(np.arange(n), np.diff(rp))]) if by_source else dict(beta=beta)
    return _case(graph, n, rp, ci, [1, n - 2], gamma, 20, 10, 41, 3, **rate)


def _events(name, rates):
    graph, seeds, sims, T, rs, off = EVENTS[name]
    n, rp, ci = _small(graph)
    beta, gamma = 0.3, 0.2
    if rates == "arrays":
        rng = np.random.default_rng(n)
        beta, gamma = rng.uniform(0.05, 0.6, n), rng.uniform(0.05, 0.6, n)
        beta[5], beta[6], gamma[7], gamma[8] = 0.0, 1.0, 0.0, 1.0
    return _case(name, n, rp, ci, seeds, gamma, sims, T, rs, off, beta=beta)


def _onehot(form):
    n, seeds = 203, [3, 77, 202]
    rp, ci = csr("er203", n, 700, 4)
    p = M.one_hot_init(n, seeds)
    if form == "scalar":
        return _case(form, n, rp, ci, p, 0.2, 40, 10, 17, 3, beta=0.3, seeds=seeds)
    rng = np.random.default_rng(6)
    w, gamma = rng.uniform(0.05, 0.9, len(ci)), rng.uniform(0.05, 0.6, n)
    w[rng.permutation(len(ci))[:len(ci) // 5]] = 0.0
    return _case(form, n, rp, ci, p if form == "p" else seeds, gamma, 40, 10, 18, 2, w=w)


def _const(i):
    graph, seeds, beta, gamma, sims, T, off = CONST[i]
    n, rp, ci = _small(graph)
    return _case(graph, n, rp, ci, seeds, gamma, sims, T, RS, off, beta=beta)


CPU_CASES = {                              # the small cases of the CPU tests
    **{f"cpu/const/{i}": functools.partial(_const, i) for i in range(len(CONST))},
    "cpu/behave": _behave,
    **{f"cpu/target/{g}": functools.partial(_target, g, False) for g in ("karate", "er200")},
    **{f"cpu/target-src/{g}": functools.partial(_target, g, True) for g in ("karate", "er200")},
    **{f"cpu/events/{g}/{r}": functools.partial(_events, g, r) for g in EVENTS for r in ("scalar", "arrays")},
    **{f"cpu/onehot/{f}": functools.partial(_onehot, f) for f in ("scalar", "seeds", "p")},
}


def _path12():
    n, rp, ci, w = M.one_way_path(12)
    return _case("path12", n, rp, ci, [5], 0.0, 7, 10, 9, w=w)


def _tree():
    n, rp, ci, w, gamma = tree_case()
    return _case("tree", n, rp, ci, tree_init(), gamma, 5000, 12, 1234, w=w)


CASES = {
    **{f"nodes/{k}": functools.partial(_shape_case, "nodes", k, live=(live_nodes, live_events)) for k in IDS},
    **{f"edges/{k}": functools.partial(_shape_case, "edges", k, live=(live_edges,)) for k in IDS},
    **{f"init/{k}": functools.partial(_shape_case, "init", k, live=(live_init,)) for k in IDS},
    # the per-trajectory tests compare the first 24 trajectories only there (the CPU side stays short)
    "nodes/wiki-vote-size/24": lambda: _shape_case("nodes", "wiki-vote-size", sims=24, live=(live_events,)),
    "nodes/large": lambda: _shape_case("nodes", "large", rng_seed=99, live=(live_events,)),
    **{f"{f}/large": functools.partial(_shape_case, f, "large", rng_seed=99) for f in ("edges", "init")},
    **{f"{f}/seeds40": functools.partial(_shape_case, f, "er-small", seeds=SEEDS40, sims=50, T=8, rng_seed=31) for f in ("nodes", "edges")},
    **{f"{f}/shard": functools.partial(_shape_case, f, "er-small", sims=40, T=12, rng_seed=5, sim_offset=600) for f in ("nodes", "edges", "init")},
    "nodes/isolated-1": lambda: _shape_case("nodes", "isolated", hetero=False),             # one seed: early extinction
    "nodes/ones": lambda: _extreme("ones", 1.0, 0.0),
    "nodes/zeros": lambda: _extreme("zeros", 0.0, 0.3),
    "nodes/almost": lambda: _extreme("almost", 1.0 - 2.0 ** -33, 0.3),
    "nodes/many": _many,
    "nodes/everybody": _everybody,
    **{f"{f}/karate": functools.partial(_karate, f) for f in ("nodes", "edges", "init")},
    **{f"init/forms-{f}": functools.partial(_init_forms, f) for f in ("scalar", "per-node", "per-node beta only")},
    "init/many": _init_many,
    "init/no-S": lambda: _init_er_small("no-S", _thirds(((0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.6, 0.4))),
                                        np.random.default_rng(9).uniform(0.05, 0.6, INIT_SHAPE["er-small"][1]), 100, 10, 51, beta=0.4),
    "init/no-I": lambda: _init_er_small("no-I", _thirds(((1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.7, 0.0, 0.3))), 0.2, 100, 10, 52, beta=0.4),
    "init/T1": lambda: _init_er_small("T1", None, 0.2, 100, 1, 53, beta=0.3),
    "init/isolated-nodes": _init_isolated_nodes,
    "init/lds64k": _init_lds64k,
    **CPU_CASES, "cpu/path12": _path12, "cpu/tree": _tree,
}


@functools.lru_cache(maxsize=None)
def case(key):
    return CASES[key]()


class Expected:
    """The model's output for a case: the events, and the counts (under the row-0 rule of the case's start) and curves folded
    from them when first asked for.  Every array is read-only."""

    def __init__(self, c):
        thr = M.infection_thresholds(c.n, c.ci, beta=c.beta, w=c.w)
        self.t_inf, self.t_rec = M.sir_events(c.n, c.rp, c.ci, c.start, thr, c.gamma, c.sims, c.T, c.rng_seed, c.sim_offset)
        self.t_inf.setflags(write=False)
        self.t_rec.setflags(write=False)
        self._T, self._seeded = c.T, np.ndim(c.start) == 1

    @functools.cached_property
    def counts(self):
        cnt = M.counts(self.t_inf, self.t_rec, self._T, hold_row0=self._seeded)
        cnt.setflags(write=False)
        return cnt

    @functools.cached_property
    def curves(self):
        cv = M.curves(self.t_inf, self.t_rec, self._T)
        cv.setflags(write=False)
        return cv


@functools.lru_cache(maxsize=None)
def expected(key):
    """`Expected` of a named case, computed once."""
    return Expected(case(key))
