"""CPU: the per-edge Monte-Carlo entries (include/gnode.h) are exported and bound, and the Python surface refuses what it
must before the library is entered (no GPU here: a stub graph is all these calls may touch)."""
import numpy as np
import pytest

from sir_cases import StubGraph as _StubGraph


@pytest.fixture(scope="module")
def lib():
    from gnode.build import build_lib
    from gnode import _lib
    build_lib()
    return _lib.load()


def test_edges_entries_exported(lib):
    from gnode import _lib
    for name in ("gnode_sir_edges_workspace_bytes", "gnode_sir_mc_philox_edges", "gnode_sir_mc_philox_traj_edges"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
    assert lib.gnode_version() == 226
    assert len(lib.gnode_sir_edges_workspace_bytes.argtypes) == 2
    assert len(lib.gnode_sir_mc_philox_edges.argtypes) == 15
    assert len(lib.gnode_sir_mc_philox_traj_edges.argtypes) == 17
    assert len(lib.gnode_sir_mc_philox_traj.argtypes) == 18              # untouched
    assert lib.gnode_sir_edges_workspace_bytes(None, 20) == 0            # no handle: no guess


def test_surface_refuses_bad_gamma_and_foreign_rates():
    from gnode.ode_nn import edge_rates, sir_counts, sir_trajectories
    g = _StubGraph()
    er = edge_rates(g, np.full(18, 0.3))
    for gamma in (1.5, float("nan"), np.full(9, 0.2), [0.2] * 9 + [-0.1]):
        with pytest.raises(ValueError):
            sir_counts(g, [0], er, gamma, sims=4, T=3, rng_seed=1)
        with pytest.raises(ValueError):
            sir_trajectories(g, [0], er, gamma, sims=4, T=3, rng_seed=1)
    other = edge_rates((np.array([0, 1, 2]), np.array([1, 0])), [0.5, 0.5])   # made for another graph
    with pytest.raises(ValueError):
        sir_counts(g, [0], other, 0.2, sims=4, T=3, rng_seed=1)


def test_sir_torch_parity_mode_refuses_edge_rates():
    import networkx as nx
    from gnode.ode_nn import edge_rates, sir_torch
    G = nx.path_graph(10)
    with pytest.raises(ValueError):
        sir_torch(G, [0], edge_rates(G, np.full(18, 0.3)), 0.2, sims=2, T=3, coins=np.full(100, 0.5))
