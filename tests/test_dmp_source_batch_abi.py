"""CPU: the batched source-inference entries (include/gnode.h) are exported and bound, `source_scores_batch` refuses what it must
before the library is loaded or a DeviceGraph is made (no GPU here: both are made to raise), `source_candidates_batch` unites
the rows' candidates and `source_rank_of` counts who beats the truth."""
import numpy as np
import pytest
import torch

from test_dmp_source_abi import A, N, OBS, Reached, lib, no_library  # noqa: F401  (the 10-node path and the two fixtures)

OBS2 = [0, 1, 2, 0, -1, 0, 0, 1, -1, 0]
ROWS = [OBS, OBS2, [-1] * N]


def test_batch_entries_exported(lib):  # noqa: F811
    from gnode import _lib
    arity = {"gnode_dmp_source_batch_tile": 1, "gnode_dmp_source_batch_workspace_bytes": 4, "gnode_dmp_source_batch_scores_f32": 14}
    for name, count in arity.items():
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
        assert len(getattr(lib, name).argtypes) == count, name
    assert lib.gnode_version() == 226                               # a stale library is known by the missing symbol


def test_queries_answer_0_without_a_handle(lib):  # noqa: F811
    assert lib.gnode_dmp_source_batch_tile(None) == 0
    for C, O, T in ((1, 1, 2), (5, 3, 8), (0, 3, 8), (5, 0, 8), (5, 3, 1), (-1, 3, 8), (5, -2, 8)):
        assert lib.gnode_dmp_source_batch_workspace_bytes(None, C, O, T) == 0


def test_source_scores_batch_refuses_before_the_library(no_library):  # noqa: F811
    from gnode.dmp import DmpGraph, source_scores_batch
    for graph in (A, DmpGraph(A)):
        shapes = (OBS, [], np.zeros((0, N), dtype=np.int8), torch.zeros((0, N), dtype=torch.int64),      # 1-D; O = 0
                  [OBS[:-1], OBS2[:-1]], [OBS + [0]], [OBS, OBS2[:-1]], [OBS, OBS2 + [0]], 1, [[OBS]])   # n - 1, n + 1, ragged
        for bad in shapes:
            with pytest.raises(ValueError):
                source_scores_batch(graph, bad, 0.3, 5)
        for value in (3, -2, 0.5, float("nan")):                    # a value outside -1 .. 2, or not whole
            bad = [[float(v) for v in row] for row in ROWS]
            bad[1][4] = value
            with pytest.raises(ValueError):
                source_scores_batch(graph, bad, 0.3, 5)
        for bad in (np.full(N - 1, 0.3), np.full(N + 1, 0.3), np.full((2, N), 0.3), [0.3] * (N - 1) + [float("nan")], -0.1, float("inf")):
            with pytest.raises(ValueError):
                source_scores_batch(graph, ROWS, bad, 5)            # gamma
        for bad in ([N], [-1], [0, N + 3], [2, 3, N], [[2, 3]], [], 2, [2.5]):           # a candidate outside the graph; shapes
            with pytest.raises(ValueError):
                source_scores_batch(graph, ROWS, 0.3, 5, candidates=bad)
        for bad in (0.0, -1e-30, 1.0 + 1e-6, 2.0, float("nan"), float("inf"), 1e-60):    # (1e-60 is 0 as a float32)
            with pytest.raises(ValueError):
                source_scores_batch(graph, ROWS, 0.3, 5, floor=bad)
        for bad in (1, 0, -3):
            with pytest.raises(ValueError):
                source_scores_batch(graph, ROWS, 0.3, bad)


def test_source_scores_batch_reaches_the_library_with_well_formed_input(no_library):  # noqa: F811
    from gnode.dmp import DmpGraph, source_scores_batch
    for graph in (A, DmpGraph(A)):
        for obs in (ROWS, np.asarray(ROWS, dtype=np.int8), torch.tensor(ROWS), [[float(v) for v in row] for row in ROWS],
                    [OBS], np.asarray([OBS]), torch.tensor([OBS], dtype=torch.int64), [[-1] * N], [[0] * N] * 2):
            for gamma in (0.3, np.full(N, 0.3), 0.0, 1.5):
                with pytest.raises(Reached):
                    source_scores_batch(graph, obs, gamma, 2)
        for cand in (None, [4], [7, 2, 2, 9], np.arange(N), torch.tensor([3, 4])):
            for floor in (1e-30, 1.0, 1e-6):
                with pytest.raises(Reached):
                    source_scores_batch(graph, ROWS, 0.3, 8, candidates=cand, floor=floor, budget_bytes=1)     # the budget needs the library


def test_default_candidates_of_a_batch():
    from gnode.dmp import source_candidates_batch
    assert source_candidates_batch(ROWS).tolist() == [1, 2, 3, 4, 7]                    # I or R in at least one row, ascending
    assert source_candidates_batch([OBS]).tolist() == [2, 3, 4]
    assert source_candidates_batch(torch.tensor(ROWS, dtype=torch.int8)).tolist() == [1, 2, 3, 4, 7]
    assert source_candidates_batch([[0, -1, 0, -1], [-1, -1, 0, 0]]).tolist() == [0, 1, 2, 3]      # none: every node


def test_source_rank_of_on_a_hand_written_table():
    from gnode.dmp import source_rank_of
    # best over time per candidate:     7     2     5     2 (again)
    scores = np.asarray([[[-9.0, -4.0, -6.0, -8.0], [-3.5, -5.0, -7.0, -2.0], [-70.0, -69.0, -69.5, -90.0], [-1.0, -30.0, -30.0, -30.0]],
                         # row 0:       -4          -2          -69         -1
                         [[-5.0, -5.0, -5.0, -5.0], [-5.0, -6.0, -7.0, -8.0], [-9.0, -5.0, -9.0, -9.0], [-4.0, -9.0, -9.0, -9.0]],
                         # row 1:       -5          -5          -5          -4      (a three-way tie under one leader)
                         [[-3.0, -2.0, -1.0, -0.5], [-8.0, -8.0, -8.0, -8.0], [-0.5, -9.0, -9.0, -9.0], [-0.25, -9.0, -9.0, -9.0]]])
    #                      row 2:       -0.5        -8          -0.5        -0.25
    cands = [7, 2, 5, 2]
    # row 0, truth 2 (its FIRST position, best -2): only the repeat's -1 is greater -> 1; truth 5: three are greater
    # row 1, truth 5 (-5): the ties at -5 do not count, the -4 does -> 1;  row 2, truth 2 (-8): all three others -> 3
    assert scores.shape == (3, 4, 4)
    for table in (scores, torch.from_numpy(scores)):
        got = source_rank_of(table, cands, [2, 5, 2])
        assert isinstance(got, torch.Tensor) and got.dtype == torch.int64 and got.tolist() == [1, 1, 3]
        assert source_rank_of(table, np.asarray(cands), torch.tensor([5, 7, 7])).tolist() == [3, 1, 1]
    assert source_rank_of(scores[:1], cands, [7]).tolist() == [2]
    for bad_truth in ([2, 5, 9], [2, 5, -1]):                       # not among the candidates
        with pytest.raises(ValueError):
            source_rank_of(scores, cands, bad_truth)
    for bad_scores, bad_cand, bad_truth in ((scores, cands[:3], [2, 5, 2]), (scores, cands, [2, 5]), (scores[0], cands, [2]),
                                            (scores[:, :, :0], cands, [2, 5, 2]), (scores, [cands], [2, 5, 2])):
        with pytest.raises(ValueError):
            source_rank_of(bad_scores, bad_cand, bad_truth)
