"""CPU: the per-trajectory model of tests/sir_events_model.py is held to the oracle -- its events, histogrammed in numpy,
are the counts of `gnode_oracle.sir_philox` (scalar rates) and of `sir_philox_nodes` (arrays), each of its curves is the
node sum of the oracle's single-trajectory call, and recovery never falls in the step of infection."""
import numpy as np
import pytest


def _cases():
    import gnode_oracle as O
    import networkx as nx
    from gnode.ode_nn import _csr_from_edges, _edge_arrays
    G = nx.karate_club_graph()
    rp, ci = _csr_from_edges(34, _edge_arrays(G))
    yield "karate", 34, rp, ci, [0, 33], 40, 12, 77, 9
    rp, ci, _ = O.er_graph(200, 800, seed=200)
    yield "er200", 200, rp, ci, [3, 150, 3], 24, 10, 5, 1000


CASES = list(_cases())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("rates", ["scalar", "arrays"])
def test_events_model_equals_oracle(case, rates):
    import gnode_oracle as O
    from sir_events_model import counts_from_events, sir_philox_events
    from sir_nodes_model import sir_philox_nodes
    name, n, rp, ci, seeds, sims, T, rs, off = case
    if rates == "scalar":
        beta, gamma = 0.3, 0.2
        want = O.sir_philox(n, rp, ci, seeds, beta, gamma, sims, T, rs, sim_offset=off)
        single = lambda s: O.sir_philox(n, rp, ci, seeds, beta, gamma, 1, T, rs, sim_offset=s)
    else:
        rng = np.random.default_rng(n)
        beta, gamma = rng.uniform(0.05, 0.6, n), rng.uniform(0.05, 0.6, n)
        beta[5], beta[6], gamma[7], gamma[8] = 0.0, 1.0, 0.0, 1.0
        want = sir_philox_nodes(n, rp, ci, seeds, beta, gamma, sims, T, rs, sim_offset=off)
        single = lambda s: sir_philox_nodes(n, rp, ci, seeds, beta, gamma, 1, T, rs, sim_offset=s)
    t_inf, t_rec, curves = sir_philox_events(n, rp, ci, seeds, beta, gamma, sims, T, rs, sim_offset=off)
    assert t_inf.dtype == np.int16 and t_inf.shape == (sims, n) and curves.shape == (sims, T, 3)
    assert want[2, -1].sum() > 0 and (t_inf == -1).any()
    assert np.array_equal(counts_from_events(t_inf, t_rec, T), want)
    k = len(set(seeds))
    for j in range(sims):
        one = single(off + j).astype(np.int64)
        node_sums = one.sum(axis=2).T                      # [T, 3]; with sims = 1 the row-0 quirk IS the initial state
        assert np.array_equal(curves[j].astype(np.int64), node_sums), (name, j)
        assert tuple(curves[j, 0]) == (n - k, k, 0)
    both = (t_inf >= 0) & (t_rec >= 0)
    assert both.any() and np.all(t_rec[both] > t_inf[both])
    assert np.all(t_inf[t_rec >= 0] >= 0)                  # nobody recovers without having been infected
    assert np.all(curves.astype(np.int64).sum(axis=2) == n)
