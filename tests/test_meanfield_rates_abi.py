"""CPU: the mean-field rates entry (include/gnode.h) is exported and bound, and `runge_kutta_order4` / `meanfield_batch`
refuse what they must before the library is loaded or a DeviceGraph is made (no GPU here: both are made to raise)."""
import numpy as np
import pytest
import scipy.sparse as sp


@pytest.fixture(scope="module")
def lib():
    from gnode.build import build_lib
    from gnode import _lib
    build_lib()
    return _lib.load()


def test_rates_entries_exported(lib):
    from gnode import _lib
    for name in ("gnode_meanfield_rates_workspace_bytes", "gnode_meanfield_rates_f64"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
    assert len(lib.gnode_meanfield_rates_workspace_bytes.argtypes) == 2
    assert len(lib.gnode_meanfield_rates_f64.argtypes) == 17
    assert len(lib.gnode_meanfield_f64.argtypes) == 16 and len(lib.gnode_meanfield_init_f64.argtypes) == 15     # untouched
    assert lib.gnode_meanfield_rates_workspace_bytes(None, 4) == 0          # no handle: no guess


N, NNZ = 10, 18
RP = np.concatenate([[0], np.cumsum([1] + [2] * 8 + [1])])
CI = np.asarray([j for i in range(N) for j in (i - 1, i + 1) if 0 <= j < N])


class _StubGraph:
    """What `meanfield_batch` reads before it enters the library.  `handle` raises: reaching it means a check came too late."""
    n, nnz, rowptr, col = N, NNZ, RP, CI

    @property
    def handle(self):
        raise AssertionError("the library was entered before the rates were checked")


@pytest.fixture
def no_library(monkeypatch):
    from gnode import _lib, ode_nn

    def refuse(*a, **k):
        raise AssertionError("the library was loaded, or a DeviceGraph made, before the rates were checked")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(ode_nn, "DeviceGraph", refuse)


def _foreign_rates():
    from gnode.ode_nn import edge_rates
    return edge_rates((np.array([0, 1, 2]), np.array([1, 0])), [0.5, 0.5])


BAD_NODE_RATES = [np.full(N - 1, 0.2), np.full(N + 1, 0.2), [0.2] * (N - 1) + [float("nan")], [0.2] * (N - 1) + [-0.1],
                  [0.2] * (N - 1) + [float("inf")], np.full((2, N), 0.2)]


def test_runge_kutta_order4_refuses_before_the_library(no_library):
    from gnode.ode_nn import InitialState, edge_rates, runge_kutta_order4, sir
    A = sp.csr_matrix((np.ones(NNZ), CI, RP), shape=(N, N))
    for bad in BAD_NODE_RATES:
        with pytest.raises(ValueError):
            runge_kutta_order4(sir, A, N, [0], bad, 0.2, 1, 5)
        with pytest.raises(ValueError):
            runge_kutta_order4(sir, A, N, [0], 0.1, bad, 1, 5)
        with pytest.raises(ValueError):
            runge_kutta_order4(sir, A, N, InitialState.from_sets(N, [0]), edge_rates((RP, CI), np.full(NNZ, 0.3)), bad, 1, 5)
    with pytest.raises(ValueError):
        runge_kutta_order4(sir, A, N, [0], _foreign_rates(), 0.2, 1, 5)
    with pytest.raises(ValueError):
        runge_kutta_order4(sir, A, N, [0], np.full(N, 0.1), float("nan"), 1, 5)         # a number beside an array is checked too
    with pytest.raises(ValueError):
        runge_kutta_order4(sir, A, N, [N], np.full(N, 0.1), 0.2, 1, 5)                  # a seed outside the graph
    with pytest.raises(AssertionError):                                                 # rates above 1 are rates: they pass
        runge_kutta_order4(sir, A, N, [0], np.full(N, 1.5), np.full(N, 2.0), 1, 5)


def test_meanfield_batch_refuses_before_the_library():
    from gnode.ode_nn import InitialState, edge_rates, meanfield_batch
    g, starts = _StubGraph(), [[0], [3, 4], InitialState.from_sets(N, [9])]
    B = len(starts)
    bad_rows = BAD_NODE_RATES[:5] + [np.full((B + 1, N), 0.2), np.full((B - 1, N), 0.2), np.full((B, N - 1), 0.2), [0.1] * (B + 1),
                                     [0.1, -0.1, 0.1], [0.1, float("nan"), 0.1]]
    nan_row = np.full((B, N), 0.2)
    nan_row[1, 4] = np.nan
    for bad in bad_rows + [nan_row, -nan_row]:
        with pytest.raises(ValueError):
            meanfield_batch(g, starts, bad, 0.2, maxTime=5)
        with pytest.raises(ValueError):
            meanfield_batch(g, starts, 0.1, bad, maxTime=5)
        with pytest.raises(ValueError):
            meanfield_batch(g, starts, edge_rates(g, np.full(NNZ, 0.3)), bad, maxTime=5)
    with pytest.raises(ValueError):
        meanfield_batch(g, starts, _foreign_rates(), 0.2, maxTime=5)
    with pytest.raises(ValueError):
        meanfield_batch(g, [], 0.1, 0.2, maxTime=5)
    with pytest.raises(ValueError):
        meanfield_batch(g, [[0], InitialState.from_sets(N - 1, [0])], 0.1, 0.2, maxTime=5)
    for ok in (np.full((B, N), 1.5), [0.1, 0.2, 0.3], np.full(N, 0.1), 0.1, edge_rates(g, np.full(NNZ, 0.3))):
        with pytest.raises(AssertionError):                                             # well-formed: the library is next
            meanfield_batch(g, starts, ok, [0.2, 0.3, 0.4], maxTime=5)
