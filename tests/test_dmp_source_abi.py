"""CPU: the source-inference entries (include/gnode.h) are exported and bound, `source_scores` refuses what it must before the
library is loaded or a DeviceGraph is made (no GPU here: both are made to raise), and `rank_sources` orders a score table."""
import numpy as np
import pytest
import scipy.sparse as sp


@pytest.fixture(scope="module")
def lib():
    from gnode.build import build_lib
    from gnode import _lib
    build_lib()
    return _lib.load()


def test_source_entries_exported(lib):
    from gnode import _lib
    for name in ("gnode_dmp_source_lds_bytes", "gnode_dmp_source_workspace_bytes", "gnode_dmp_source_scores_f32"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
    assert len(lib.gnode_dmp_source_lds_bytes.argtypes) == 1
    assert len(lib.gnode_dmp_source_workspace_bytes.argtypes) == 3
    assert len(lib.gnode_dmp_source_scores_f32.argtypes) == 12
    assert lib.gnode_version() == 226                               # a stale library is known by the missing symbol


def test_size_queries_answer_0_without_a_handle(lib):
    assert lib.gnode_dmp_source_lds_bytes(None) == 0
    for C, T in ((1, 2), (5, 8), (0, 8), (5, 1)):
        assert lib.gnode_dmp_source_workspace_bytes(None, C, T) == 0


N, NNZ = 10, 18
RP = np.concatenate([[0], np.cumsum([1] + [2] * 8 + [1])])
CI = np.asarray([j for i in range(N) for j in (i - 1, i + 1) if 0 <= j < N])
A = sp.csr_matrix((np.linspace(0.1, 0.5, NNZ), CI, RP), shape=(N, N))
OBS = [0, 0, 1, 2, 1, 0, -1, 0, 0, -1]


class Reached(Exception):
    pass


@pytest.fixture
def no_library(monkeypatch):
    from gnode import _lib, dmp

    def refuse(*a, **k):
        raise Reached("the library was loaded, or a DeviceGraph made")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(dmp, "DeviceGraph", refuse)


def test_source_scores_refuses_before_the_library(no_library):
    from gnode.dmp import DmpGraph, source_scores
    for graph in (A, DmpGraph(A)):
        for bad in (OBS[:-1], OBS + [0], [OBS], [], 1):                                 # shapes of obs
            with pytest.raises(ValueError):
                source_scores(graph, bad, 0.3, 5)
        for value in (3, -2, 7, 0.5, float("nan")):                                     # an obs value outside -1 .. 2, or not whole
            bad = [float(v) for v in OBS]
            bad[4] = value
            with pytest.raises(ValueError):
                source_scores(graph, bad, 0.3, 5)
        for bad in (np.full(N - 1, 0.3), np.full(N + 1, 0.3), np.full((2, N), 0.3), [0.3] * (N - 1) + [float("nan")], -0.1, float("inf")):
            with pytest.raises(ValueError):
                source_scores(graph, OBS, bad, 5)                                       # gamma
        for bad in ([N], [-1], [0, N + 3], [2, 3, N], [[2, 3]], [], 2, [2.5]):           # a candidate outside the graph; shapes
            with pytest.raises(ValueError):
                source_scores(graph, OBS, 0.3, 5, candidates=bad)
        for bad in (0.0, -1e-30, 1.0 + 1e-6, 2.0, float("nan"), float("inf"), 1e-60):    # (1e-60 is 0 as a float32)
            with pytest.raises(ValueError):
                source_scores(graph, OBS, 0.3, 5, floor=bad)
        for bad in (1, 0, -3):
            with pytest.raises(ValueError):
                source_scores(graph, OBS, 0.3, bad)


def test_source_scores_reaches_the_library_with_well_formed_input(no_library):
    import torch
    from gnode.dmp import DmpGraph, source_scores
    for graph in (A, DmpGraph(A)):
        for obs in (OBS, np.asarray(OBS), np.asarray(OBS, dtype=np.int8), torch.tensor(OBS), [float(v) for v in OBS], [-1] * N, [0] * N):
            for gamma in (0.3, np.full(N, 0.3), 0.0, 1.5):
                with pytest.raises(Reached):
                    source_scores(graph, obs, gamma, 2)
        for cand in (None, [4], [7, 2, 2, 9], np.arange(N), torch.tensor([3, 4])):
            for floor in (1e-30, 1.0, 1e-6):
                with pytest.raises(Reached):
                    source_scores(graph, OBS, 0.3, 8, candidates=cand, floor=floor, budget_bytes=1)     # the budget needs the library


def test_default_candidates():
    from gnode.dmp import source_candidates
    assert source_candidates(OBS).tolist() == [2, 3, 4]            # observed infected or recovered: a source is not susceptible
    assert source_candidates([0, -1, 0, -1]).tolist() == [0, 1, 2, 3]                    # none: every node


def test_rank_sources_on_a_hand_written_table():
    import torch
    from gnode.dmp import rank_sources
    scores = np.asarray([[-9.0, -4.0, -6.0, -8.0],                   # candidate 7: best -4 at t = 1
                         [-3.5, -5.0, -7.0, -2.0],                   # candidate 2: best -2 at t = 3
                         [-70.0, -69.0, -69.5, -90.0],               # candidate 5: best -69 at t = 1
                         [-3.0, -30.0, -30.0, -30.0]])               # candidate 0: best -3 at t = 0
    want = [(2, 3, -2.0), (0, 0, -3.0), (7, 1, -4.0), (5, 1, -69.0)]
    assert rank_sources(scores, [7, 2, 5, 0]) == want
    assert rank_sources(torch.from_numpy(scores), np.asarray([7, 2, 5, 0])) == want
    assert rank_sources(scores[:1], [7]) == [(7, 1, -4.0)]
    for bad_scores, bad_cand in ((scores, [7, 2, 5]), (scores[0], [7]), (scores[:, :0], [7, 2, 5, 0])):
        with pytest.raises(ValueError):
            rank_sources(bad_scores, bad_cand)
