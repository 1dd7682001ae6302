"""CPU: the outbreak-size entries (include/gnode.h) are exported and bound, `outbreak_sizes` and the greedy helpers refuse what
they must before the library is loaded or a DeviceGraph is made (no GPU here: both are made to raise), and `infections` reads a
hand-written table."""
import numpy as np
import pytest
import scipy.sparse as sp


@pytest.fixture(scope="module")
def lib():
    from gnode.build import build_lib
    from gnode import _lib
    build_lib()
    return _lib.load()


def test_outbreak_entries_exported(lib):
    from gnode import _lib
    for name in ("gnode_dmp_outbreak_lds_bytes", "gnode_dmp_outbreak_workspace_bytes", "gnode_dmp_outbreak_sizes_f32"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
    assert len(lib.gnode_dmp_outbreak_lds_bytes.argtypes) == 1
    assert len(lib.gnode_dmp_outbreak_workspace_bytes.argtypes) == 3
    assert len(lib.gnode_dmp_outbreak_sizes_f32.argtypes) == 13
    assert lib.gnode_version() == 226                               # a stale library is known by the missing symbol


def test_size_queries_answer_0_without_a_handle(lib):
    assert lib.gnode_dmp_outbreak_lds_bytes(None) == 0
    for C, T in ((1, 2), (5, 8), (0, 8), (5, 1)):
        assert lib.gnode_dmp_outbreak_workspace_bytes(None, C, T) == 0


N, NNZ = 10, 18
RP = np.concatenate([[0], np.cumsum([1] + [2] * 8 + [1])])
CI = np.asarray([j for i in range(N) for j in (i - 1, i + 1) if 0 <= j < N])
A = sp.csr_matrix((np.linspace(0.1, 0.5, NNZ), CI, RP), shape=(N, N))


class Reached(Exception):
    pass


@pytest.fixture
def no_library(monkeypatch):
    from gnode import _lib, dmp

    def refuse(*a, **k):
        raise Reached("the library was loaded, or a DeviceGraph made")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(dmp, "DeviceGraph", refuse)


BAD_GAMMA = (np.full(N - 1, 0.3), np.full(N + 1, 0.3), np.full((2, N), 0.3), [0.3] * (N - 1) + [float("nan")], -0.1, float("inf"), "x")
BAD_VALUE = (np.ones(N - 1), np.ones(N + 1), np.ones((1, N)), 1.0, [1.0] * (N - 1) + [-0.5], [1.0] * (N - 1) + [float("nan")],
             [1.0] * (N - 1) + [float("inf")])
BAD_START = ([N], [-1], [0, N + 3], [[2, 3]], 2, [2.5], "ab")
BAD_CANDIDATES = ([N], [-2], [0, N + 3], [2, 3, N], [[2, 3]], [], 2, [2.5])


def _mixed(n):
    from gnode.ode_nn import initial_state
    return initial_state(np.random.default_rng(1).dirichlet([4, .5, .5], n))


def test_outbreak_sizes_refuses_before_the_library(no_library):
    from gnode.dmp import DmpGraph, outbreak_sizes
    from gnode.ode_nn import InitialState
    for graph in (A, DmpGraph(A)):
        for bad in BAD_GAMMA:
            with pytest.raises(ValueError):
                outbreak_sizes(graph, bad, 5, start=[0])
        for bad in BAD_VALUE:
            with pytest.raises(ValueError):
                outbreak_sizes(graph, 0.3, 5, start=[0], value=bad)
        for bad in BAD_START + (_mixed(N - 1), _mixed(N + 1)):
            with pytest.raises(ValueError):
                outbreak_sizes(graph, 0.3, 5, start=bad)
        for bad in BAD_CANDIDATES:
            with pytest.raises(ValueError):
                outbreak_sizes(graph, 0.3, 5, candidates=bad, start=[0])
        for bad in ("vaccinate", "Seed", 0, None, ""):               # an unknown action
            with pytest.raises(ValueError):
                outbreak_sizes(graph, 0.3, 5, action=bad, start=[0])
        for start in (None, [], InitialState.from_sets(N, [], [3])):  # nothing infected: nothing to immunise against
            with pytest.raises(ValueError):
                outbreak_sizes(graph, 0.3, 5, action="immunise", start=start)
        for bad in (1, 0, -3):
            with pytest.raises(ValueError):
                outbreak_sizes(graph, 0.3, bad, start=[0])


def test_greedy_helpers_refuse_before_the_library(no_library):
    from gnode.dmp import DmpGraph, greedy_immunisation, greedy_seeds
    from gnode.ode_nn import InitialState
    for graph in (A, DmpGraph(A)):
        for bad in BAD_GAMMA:
            with pytest.raises(ValueError):
                greedy_immunisation(graph, [0], bad, 5, 1)
            with pytest.raises(ValueError):
                greedy_seeds(graph, bad, 5, 1)
        for bad in BAD_VALUE:
            with pytest.raises(ValueError):
                greedy_immunisation(graph, [0], 0.3, 5, 1, value=bad)
            with pytest.raises(ValueError):
                greedy_seeds(graph, 0.3, 5, 1, value=bad)
        for bad in BAD_START:
            with pytest.raises(ValueError):
                greedy_immunisation(graph, bad, 0.3, 5, 1)
            with pytest.raises(ValueError):
                greedy_seeds(graph, 0.3, 5, 1, start=bad)
        for bad in BAD_CANDIDATES + ([-1], [3, -1]):                 # "no change" is no node to choose
            with pytest.raises(ValueError):
                greedy_immunisation(graph, [0], 0.3, 5, 1, candidates=bad)
            with pytest.raises(ValueError):
                greedy_seeds(graph, 0.3, 5, 1, candidates=bad)
        for start in (None, [], InitialState.from_sets(N, [], [3])):
            with pytest.raises(ValueError):
                greedy_immunisation(graph, start, 0.3, 5, 1)
        for bad in (1, 0, -3):
            with pytest.raises(ValueError):
                greedy_immunisation(graph, [0], 0.3, bad, 1)
            with pytest.raises(ValueError):
                greedy_seeds(graph, 0.3, bad, 1)
        # k: at least 1, whole, and no more than the candidates that are still susceptible in the start
        for k in (0, -1, 1.5, None, "2", N):                        # (node 0 is infected: N - 1 are left)
            with pytest.raises(ValueError):
                greedy_immunisation(graph, [0], 0.3, 5, k)
        for k in (0, -2, N + 1):
            with pytest.raises(ValueError):
                greedy_seeds(graph, 0.3, 5, k)
        with pytest.raises(ValueError):
            greedy_seeds(graph, 0.3, 5, 3, candidates=[4, 7, 4])    # two distinct candidates
        with pytest.raises(ValueError):
            greedy_immunisation(graph, InitialState.from_sets(N, [0], [4]), 0.3, 5, 2, candidates=[0, 4, 7])    # one left


def test_well_formed_input_reaches_the_library(no_library):
    import torch
    from gnode.dmp import DmpGraph, greedy_immunisation, greedy_seeds, outbreak_sizes
    from gnode.ode_nn import InitialState
    for graph in (A, DmpGraph(A)):
        for gamma in (0.3, np.full(N, 0.3), 0.0, 1.5, torch.full((N,), 0.3)):
            for value in (None, np.ones(N), [0.0] * N, torch.arange(N)):
                with pytest.raises(Reached):
                    outbreak_sizes(graph, gamma, 2, value=value)
        for start in (None, [], [0], [3, 3, 9], np.asarray([2]), _mixed(N), InitialState.from_sets(N, [1], [2])):
            for cand in (None, [4], [7, 2, 2, 9, -1], [-1], np.arange(N), torch.tensor([3, 4])):
                with pytest.raises(Reached):
                    outbreak_sizes(graph, 0.3, 8, candidates=cand, action="seed", start=start, budget_bytes=1)   # the budget needs the library
        for start in ([0], _mixed(N), InitialState.from_sets(N, [1], [2])):
            with pytest.raises(Reached):
                outbreak_sizes(graph, 0.3, 8, candidates=[-1, 5], action="immunise", start=start)
            for k in (1, 3, np.int64(2), 2.0):
                with pytest.raises(Reached):
                    greedy_immunisation(graph, start, 0.3, 8, k)
        for k, cand in ((1, None), (N, None), (2, [4, 7, 4]), (1, [0])):
            with pytest.raises(Reached):
                greedy_seeds(graph, 0.3, 8, k, candidates=cand)
        with pytest.raises(Reached):
            greedy_seeds(graph, 0.3, 8, N - 1, start=[0])


def test_infections_on_a_hand_written_table():
    import torch
    from gnode.dmp import infections
    sizes = np.asarray([[[9.0, 1.0, 0.0], [7.5, 2.0, 0.5], [6.0, 2.25, 1.75]],        # nobody removed at the start: 2.25 + 1.75
                        [[8.0, 1.0, 1.0], [7.0, 1.5, 1.5], [6.5, 1.0, 2.5]]])         # one immunised: 1.0 + 2.5 - 1.0
    want = [4.0, 2.5]
    got = infections(sizes)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.tolist() == want
    got = infections(torch.from_numpy(sizes))
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float64 and got.tolist() == want
    assert infections(sizes[:1, :1]).tolist() == [1.0 + 0.0 - 0.0]   # a horizon of one row: the start's infected
    for bad in (sizes[0], sizes[:, :, :2], sizes[:, :0], 3.0):
        with pytest.raises(ValueError):
            infections(bad)
