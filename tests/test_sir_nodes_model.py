"""CPU: the per-node-rate model of tests/sir_nodes_model.py held to the existing oracle (`sir_philox`) and to what the
rates mean, so that a wrong helper cannot bless a wrong kernel (tests/test_gpu_sir_nodes.py compares the GPU with it)."""
import numpy as np
import pytest


def _karate():
    import networkx as nx
    import gnode_oracle as O
    G = nx.karate_club_graph()
    return (34, *O.csr_from_edges(34, [(int(a), int(b)) for a, b in G.edges()]))


def _er200():
    import gnode_oracle as O
    rp, ci, _ = O.er_graph(200, 800, seed=200)
    return 200, rp, ci


@pytest.mark.parametrize("graph,seeds,beta,gamma,sims,T,off", [
    (_karate, [0, 33], 0.3, 0.2, 40, 12, 0),
    (_er200, [3, 150], 0.45, 0.15, 24, 10, 0),
    (_er200, [3, 150], 0.05, 0.6, 24, 10, 1000),       # sim_offset: other trajectories' coins
    (_karate, [5], 1.0, 0.0, 6, 6, 7),                 # the two ends of the threshold range
])
def test_constant_arrays_equal_scalar_oracle(graph, seeds, beta, gamma, sims, T, off):
    import gnode_oracle as O
    from sir_nodes_model import sir_philox_nodes
    n, rp, ci = graph()
    want = O.sir_philox(n, rp, ci, seeds, beta, gamma, sims, T, rng_seed=0xABCDEF0123, sim_offset=off)
    assert want[2, -1].sum() > 0 or gamma == 0.0
    for b, g in ((np.full(n, beta), np.full(n, gamma)), (beta, np.full(n, gamma)), (np.full(n, beta), gamma)):
        assert np.array_equal(sir_philox_nodes(n, rp, ci, seeds, b, g, sims, T, rng_seed=0xABCDEF0123, sim_offset=off), want)


def test_edge_rates_behave():
    """beta_v = 0 nodes never leave S, gamma_u = 1 nodes are in I for exactly one step, gamma_u = 0 nodes never reach R,
    and every trajectory has every node in exactly one compartment."""
    from sir_nodes_model import sir_philox_nodes
    n, rp, ci = _er200()
    rng = np.random.default_rng(7)
    beta, gamma = rng.uniform(0.2, 0.7, n), rng.uniform(0.1, 0.5, n)
    seeds = [3, 150]
    pos = rng.permutation(np.setdiff1d(np.arange(n), seeds))
    b0, g1, g0 = pos[:20], pos[20:40], pos[40:60]
    beta[b0], gamma[g1], gamma[g0] = 0.0, 1.0, 0.0
    sims, T = 30, 14
    c = sir_philox_nodes(n, rp, ci, seeds, beta, gamma, sims, T, rng_seed=99).astype(np.int64)
    assert np.all(c[0, 1:] + c[1, 1:] + c[2, 1:] == sims)
    assert np.all(c[0, 1:, b0] == sims)                                   # shielded: susceptible for ever
    ever = sims - c[0, -1]                                                # trajectories in which the node was infected
    assert ever[g1].sum() > 0 and ever[g0].sum() > 0                      # (the epidemic did reach such nodes)
    # gamma = 1: a node infected at step t is in I at t and in R from t + 1 on, so over all steps its I count sums to
    # one per infection that happened before the last step
    inf_before_last = sims - c[0, -2]
    assert np.array_equal(c[1, 1:-1].sum(0)[g1], inf_before_last[g1])
    assert np.array_equal(c[2, -1][g1], inf_before_last[g1])
    assert not c[2][:, g0].any()                                          # gamma = 0: never recovered
    assert np.array_equal(c[1, -1][g0], ever[g0])                         # ... still infected at the end
