"""CPU: the batched DMP entries (include/gnode.h) are exported and bound, and `dmp_batch` refuses what it must before the
library is loaded or a DeviceGraph is made (no GPU here: both are made to raise)."""
import numpy as np
import pytest
import scipy.sparse as sp


@pytest.fixture(scope="module")
def lib():
    from gnode.build import build_lib
    from gnode import _lib
    build_lib()
    return _lib.load()


def test_batch_entries_exported(lib):
    from gnode import _lib
    for name in ("gnode_dmp_batch_workspace_bytes", "gnode_dmp_batch_lds_bytes", "gnode_dmp_batch_f32"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
    assert len(lib.gnode_dmp_batch_workspace_bytes.argtypes) == 2
    assert len(lib.gnode_dmp_batch_lds_bytes.argtypes) == 1
    assert len(lib.gnode_dmp_batch_f32.argtypes) == 12
    assert len(lib.gnode_dmp_f32.argtypes) == 10 and len(lib.gnode_dmp_init_f32.argtypes) == 9          # untouched
    assert lib.gnode_dmp_batch_workspace_bytes(None, 4) == 0 and lib.gnode_dmp_batch_lds_bytes(None) == 0    # no handle: no guess


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


def _starts():
    from gnode.ode_nn import InitialState
    return [[0], [3, 4], InitialState.from_sets(N, [9])]


def test_dmp_batch_refuses_before_the_library(no_library):
    from gnode.dmp import dmp_batch
    from gnode.ode_nn import InitialState
    starts = _starts()
    B = len(starts)
    with pytest.raises(ValueError):
        dmp_batch(A, [], 0.2, 5)                                                        # an empty batch
    with pytest.raises(ValueError):
        dmp_batch(A, [[0], InitialState.from_sets(N - 1, [0])], 0.2, 5)                 # a state of another graph
    for seeds in ([N], [-1], [0, N + 3]):
        with pytest.raises(ValueError):
            dmp_batch(A, [[0], seeds], 0.2, 5)                                          # a seed outside the graph
    nan_rows = np.full((B, N), 0.2)
    nan_rows[1, 4] = np.nan
    bad_gamma = [np.full(N - 1, 0.2), np.full(N + 1, 0.2), np.full((B + 1, N), 0.2), np.full((B - 1, N), 0.2), np.full((B, N - 1), 0.2),
                 [0.1] * (B + 1), np.full((1, B, N), 0.2), [0.2] * (N - 1) + [float("nan")], [0.2] * (N - 1) + [-0.1],
                 [0.2] * (N - 1) + [float("inf")], [0.1, -0.1, 0.1], [0.1, float("nan"), 0.1], nan_rows, -nan_rows, float("nan"), -0.5,
                 float("inf")]
    for bad in bad_gamma:
        with pytest.raises(ValueError):
            dmp_batch(A, starts, bad, 5)
        with pytest.raises(ValueError):
            dmp_batch(A, starts, bad, 5, scale=[1.0, 0.5, 0.25])
    bad_scale = [0.5, [0.5] * (B + 1), [0.5] * (B - 1), np.full((B, NNZ), 0.5), [0.5, float("nan"), 0.5], [0.5, -0.5, 0.5],
                 [0.5, float("inf"), 0.5], []]
    for bad in bad_scale:
        with pytest.raises(ValueError):
            dmp_batch(A, starts, 0.2, 5, scale=bad)


def test_dmp_batch_reaches_the_library_with_well_formed_input(no_library):
    from gnode.dmp import DmpGraph, dmp_batch
    starts = _starts()
    B = len(starts)
    for gamma in (0.2, np.full(N, 0.2), np.full((B, N), 0.2), [0.1, 0.2, 0.3], 1.5, 0.0):
        for scale in (None, [1.0, 0.5, 0.0], np.asarray([2.0, 1.0, 0.5])):
            with pytest.raises(Reached):
                dmp_batch(A, starts, gamma, 5, scale=scale)
    with pytest.raises(Reached):
        dmp_batch(DmpGraph(A), starts, 0.2, 5)                      # a prepared graph makes its handle on first use, not before
    with pytest.raises(Reached):
        dmp_batch(A, [[0]] * N, np.linspace(0.1, 0.4, N), 5)        # B == n: a 1-D gamma of length n is per node
