"""CPU: the initial-state entries (include/gnode.h) are exported and bound, and the Python surface refuses what it must
before the library is entered (no GPU here: a stub graph is all these calls may touch)."""
import numpy as np
import pytest

from sir_cases import StubGraph as _StubGraph


@pytest.fixture(scope="module")
def lib():
    from gnode.build import build_lib
    from gnode import _lib
    build_lib()
    return _lib.load()


def test_init_entries_exported(lib):
    from gnode import _lib
    want = {"gnode_sir_init_workspace_bytes": 2, "gnode_sir_mc_philox_init": 18, "gnode_dmp_init_workspace_bytes": 1,
            "gnode_dmp_init_f32": 9, "gnode_meanfield_init_f64": 15}
    for name, n_args in want.items():
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
        assert len(getattr(lib, name).argtypes) == n_args, name
    assert lib.gnode_version() == 226
    assert len(lib.gnode_sir_mc_philox_traj.argtypes) == 18              # untouched
    assert len(lib.gnode_sir_mc_philox_edges.argtypes) == 15
    assert len(lib.gnode_dmp_f32.argtypes) == 10
    assert len(lib.gnode_meanfield_f64.argtypes) == 16
    assert lib.gnode_sir_init_workspace_bytes(None, 20) == 0             # no handle: no guess
    assert lib.gnode_dmp_init_workspace_bytes(None) == 0


def _good(n=10):
    p = np.zeros((n, 3))
    p[:, 0] = 1.0
    p[3] = (0.2, 0.5, 0.3)
    return p


def test_initial_state_checks():
    import torch
    from gnode.ode_nn import InitialState, initial_state
    st = initial_state(_good())
    assert st.n == 10 and st.p.dtype == np.float64 and st.p.flags.c_contiguous and st.p.shape == (10, 3)
    assert np.array_equal(initial_state(_good().tolist()).p, st.p)
    x = torch.zeros(10, 8)
    x[:, :3] = torch.from_numpy(_good()).float()
    assert np.allclose(initial_state(x[:, :3]).p, st.p, atol=1e-7)       # float32 columns pass the 1e-6 row-sum check
    for v in (float("nan"), -0.1, 1.5):
        p = _good()
        p[4, 1] = v
        with pytest.raises(ValueError, match=r"p\[4\]\[1\]"):
            initial_state(p)
    p = _good()
    p[6] = (0.5, 0.3, 0.21)                                              # sums to 1.01
    with pytest.raises(ValueError, match="node 6 "):
        initial_state(p)
    for shape in ((10, 2), (10,), (3, 10), (2, 10, 3)):
        with pytest.raises(ValueError):
            initial_state(np.zeros(shape))
    fs = InitialState.from_sets(10, [1, 5], immune=[7])
    assert fs.p[1].tolist() == [0, 1, 0] and fs.p[7].tolist() == [0, 0, 1] and fs.p[0].tolist() == [1, 0, 0]
    with pytest.raises(ValueError):
        InitialState.from_sets(10, [10])
    with pytest.raises(ValueError):
        InitialState.from_sets(10, [1], immune=[1])


def test_sample_tensor_columns():
    from gnode.ode_nn import InitialState, initial_state
    from gnode.trainer import sample_tensor
    assert InitialState.from_sets(10, [1, 5]).x(6, 0.3, 0.2).equal(sample_tensor(10, 6, [1, 5], 0.3, 0.2))
    x = initial_state(_good()).x(6, 0.3, 0.2)
    assert x.shape == (10, 9) and x.dtype.is_floating_point and x.element_size() == 4
    assert np.array_equal(x[:, :3].numpy(), _good().astype(np.float32)) and not x[:, 5:].any()


def test_surface_refuses_before_the_library_is_entered():
    from gnode.ode_nn import edge_rates, initial_state, sir_counts, sir_trajectories
    g = _StubGraph()
    wrong_n = initial_state(_good(9))
    for call in (sir_counts, sir_trajectories):
        with pytest.raises(ValueError):
            call(g, wrong_n, 0.3, 0.2, sims=4, T=3, rng_seed=1)
        with pytest.raises(ValueError):
            call(g, wrong_n, edge_rates(g, np.full(18, 0.3)), 0.2, sims=4, T=3, rng_seed=1)
        with pytest.raises(ValueError):                                   # a good state, a bad rate
            call(g, initial_state(_good()), 0.3, [0.2] * 9 + [1.5], sims=4, T=3, rng_seed=1)


def test_baselines_refuse_a_wrong_n():
    import scipy.sparse as sp
    from gnode import ode_nn
    from gnode.dmp import DMP_SIR
    g = _StubGraph()
    A = sp.csr_matrix((np.ones(18), g.col, g.rowptr), shape=(10, 10))
    with pytest.raises(ValueError):
        ode_nn.runge_kutta_order4(ode_nn.sir, A, 10, ode_nn.initial_state(_good(9)), 0.1, 0.2)
    m = DMP_SIR.__new__(DMP_SIR)                                          # (the constructor uploads a graph)
    m.N = 10
    with pytest.raises(ValueError):
        m.run(ode_nn.initial_state(_good(9)), 5)


def test_sir_torch_parity_mode_refuses_an_initial_state():
    import networkx as nx
    from gnode.ode_nn import InitialState, sir_torch
    G = nx.path_graph(10)
    with pytest.raises(ValueError):
        sir_torch(G, InitialState.from_sets(10, [0]), 0.3, 0.2, sims=2, T=3, coins=np.full(100, 0.5))
