"""CPU: the per-node-rate Monte-Carlo entry (include/gnode.h, ABI 226) is exported and bound, and the Python surface
refuses bad rate arrays before the library is entered (no GPU here: a stub graph is all these calls may touch)."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from gnode.build import build_lib
    from gnode import _lib
    build_lib()
    return _lib.load()


def test_nodes_entries_exported(lib):
    from gnode import _lib
    for name in ("gnode_sir_nodes_workspace_bytes", "gnode_sir_mc_philox_nodes"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
    assert lib.gnode_version() == 226
    assert len(lib.gnode_sir_mc_philox_nodes.argtypes) == 14
    assert lib.gnode_sir_nodes_workspace_bytes(None, 20) == 0          # no handle: no guess


class _StubGraph:
    """What sir_counts reads before it enters the library.  `handle` raises: reaching it means the check came too late."""
    n = 10

    @property
    def handle(self):
        raise AssertionError("the library was entered before the rates were checked")


def _bad_rates():
    ok = np.full(10, 0.3)
    yield "wrong length", np.full(9, 0.3)
    yield "two-dimensional", np.full((10, 1), 0.3)
    for what, x in (("negative", -0.1), ("above one", 1.5), ("NaN", float("nan"))):
        a = ok.copy()
        a[6] = x
        yield what, a


@pytest.mark.parametrize("what,bad", list(_bad_rates()), ids=[w for w, _ in _bad_rates()])
@pytest.mark.parametrize("as_type", ["numpy", "list", "torch"])
def test_sir_counts_refuses_bad_rates(what, bad, as_type):
    import torch
    from gnode.ode_nn import sir_counts
    conv = {"numpy": lambda a: a, "list": lambda a: a.tolist(), "torch": lambda a: torch.from_numpy(a)}[as_type]
    for kw in ({"beta": conv(bad), "gamma": 0.2}, {"beta": 0.3, "gamma": conv(bad)}, {"beta": conv(np.full(10, 0.3)), "gamma": conv(bad)}):
        with pytest.raises(ValueError):
            sir_counts(_StubGraph(), [0], sims=4, T=3, rng_seed=1, **kw)
    # the scalar side of a mixed call is checked with the array
    with pytest.raises(ValueError):
        sir_counts(_StubGraph(), [0], conv(np.full(10, 0.3)), 1.5, sims=4, T=3, rng_seed=1)


def test_sir_torch_parity_mode_takes_scalars_only():
    import networkx as nx
    from gnode.ode_nn import sir_torch
    G = nx.path_graph(10)
    coins = np.full(100, 0.5)
    with pytest.raises(ValueError):
        sir_torch(G, [0], np.full(10, 0.3), 0.2, sims=2, T=3, coins=coins)
    with pytest.raises(ValueError):
        sir_torch(G, [0], 0.3, [0.2] * 10, sims=2, T=3, coins=coins)
