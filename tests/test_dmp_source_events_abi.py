"""CPU: the event-row source-inference entries (include/gnode.h) are exported and bound, `source_scores_events` refuses what it
must before the library is loaded or a DeviceGraph is made (no GPU here: both are made to raise), `timed_observations` packs
records into rows deterministically, `observations_from_events` reads a trajectory's event steps, and the shift-and-add of
`source_scores_timed` (`sum_timed_rows`) is the explicit adds in ascending row order."""
import math

import numpy as np
import pytest
import torch

from test_dmp_source_abi import A, N, OBS, Reached, lib, no_library  # noqa: F401  (the 10-node path and the two fixtures)

OBS2 = [0, 3, 2, 0, -1, 4, 0, 1, -1, 0]
ROWS = [OBS, OBS2, [-1] * N]


def test_events_entries_exported(lib):  # noqa: F811
    from gnode import _lib
    arity = {"gnode_dmp_source_events_tile": 1, "gnode_dmp_source_events_workspace_bytes": 4, "gnode_dmp_source_events_scores_f32": 14}
    for name, count in arity.items():
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
        assert len(getattr(lib, name).argtypes) == count, name
    assert lib.gnode_version() == 226                               # a stale library is known by the missing symbol


def test_queries_answer_0_without_a_handle(lib):  # noqa: F811
    assert lib.gnode_dmp_source_events_tile(None) == 0
    for C, R, T in ((1, 1, 2), (5, 3, 8), (0, 3, 8), (5, 0, 8), (5, 3, 1), (-1, 3, 8), (5, -2, 8)):
        assert lib.gnode_dmp_source_events_workspace_bytes(None, C, R, T) == 0


def test_source_scores_events_refuses_before_the_library(no_library):  # noqa: F811
    from gnode.dmp import DmpGraph, source_scores_events
    for graph in (A, DmpGraph(A)):
        shapes = (OBS, [], np.zeros((0, N), dtype=np.int8), torch.zeros((0, N), dtype=torch.int64),      # 1-D; R = 0
                  [OBS[:-1], OBS2[:-1]], [OBS + [0]], [OBS, OBS2[:-1]], [OBS, OBS2 + [0]], 1, [[OBS]])   # n - 1, n + 1, ragged
        for bad in shapes:
            with pytest.raises(ValueError):
                source_scores_events(graph, bad, 0.3, 5)
        for value in (5, -2, 0.5, float("nan")):                    # a code outside -1 .. 4, or not whole
            bad = [[float(v) for v in row] for row in ROWS]
            bad[1][4] = value
            with pytest.raises(ValueError):
                source_scores_events(graph, bad, 0.3, 5)
        for bad in (np.full(N - 1, 0.3), np.full(N + 1, 0.3), np.full((2, N), 0.3), [0.3] * (N - 1) + [float("nan")], -0.1, float("inf")):
            with pytest.raises(ValueError):
                source_scores_events(graph, ROWS, bad, 5)           # gamma
        for bad in ([N], [-1], [0, N + 3], [2, 3, N], [[2, 3]], [], 2, [2.5]):           # a candidate outside the graph; shapes
            with pytest.raises(ValueError):
                source_scores_events(graph, ROWS, 0.3, 5, candidates=bad)
        for bad in (0.0, -1e-30, 1.0 + 1e-6, 2.0, float("nan"), float("inf"), 1e-60):    # (1e-60 is 0 as a float32)
            with pytest.raises(ValueError):
                source_scores_events(graph, ROWS, 0.3, 5, floor=bad)
        for bad in (1, 0, -3):
            with pytest.raises(ValueError):
                source_scores_events(graph, ROWS, 0.3, bad)


def test_source_scores_events_reaches_the_library_with_well_formed_input(no_library):  # noqa: F811
    from gnode.dmp import DmpGraph, source_scores_events, source_scores_timed, timed_observations
    for graph in (A, DmpGraph(A)):
        for rows in (ROWS, np.asarray(ROWS, dtype=np.int8), torch.tensor(ROWS), [[float(v) for v in row] for row in ROWS],
                     [OBS2], np.asarray([OBS2]), torch.tensor([OBS2], dtype=torch.int64), [[-1] * N], [[3] * N, [4] * N]):
            for gamma in (0.3, np.full(N, 0.3), 0.0, 1.5):
                with pytest.raises(Reached):
                    source_scores_events(graph, rows, gamma, 2)
        for cand in (None, [4], [7, 2, 2, 9], np.arange(N), torch.tensor([3, 4])):
            for floor in (1e-30, 1.0, 1e-6):
                with pytest.raises(Reached):
                    source_scores_events(graph, ROWS, 0.3, 8, candidates=cand, floor=floor, budget_bytes=1)    # the budget needs the library
        with pytest.raises(Reached):
            source_scores_timed(graph, timed_observations(N, [2, 5], [0, -3], [3, 4]), 0.3, 8)
        for bad in (ROWS, np.asarray(ROWS), None):                  # rows are not packed records
            with pytest.raises(ValueError):
                source_scores_timed(graph, bad, 0.3, 8)


def test_default_candidates_of_event_rows():
    from gnode.dmp import source_candidates_events
    assert source_candidates_events(ROWS).tolist() == [1, 2, 3, 4, 5, 7]                 # a code >= 1 in at least one row, ascending
    assert source_candidates_events([OBS2]).tolist() == [1, 2, 5, 7]
    assert source_candidates_events(torch.tensor(ROWS, dtype=torch.int8)).tolist() == [1, 2, 3, 4, 5, 7]
    assert source_candidates_events([[0, -1, 0, -1], [-1, -1, 0, 0]]).tolist() == [0, 1, 2, 3]     # none: every node


def test_timed_observations_packs_records_into_rows():
    from gnode.dmp import timed_observations
    # record:  0   1   2   3   4   5   6   7
    nodes = [4, 1, 4, 2, 1, 4, 0, 2]
    offsets = [-3, 0, -3, 0, -3, -3, 0, -7]
    kinds = [3, 0, 0, 2, 4, 1, 0, 3]
    obs = timed_observations(6, nodes, offsets, kinds)
    # offset 0 first: one row (records 1, 3, 6); offset -3: node 4 has three records, so three rows (0 and 4 | 2 | 5); offset -7
    want = [[0, 0, 2, -1, -1, -1],
            [-1, 4, -1, -1, 3, -1],
            [-1, -1, -1, -1, 0, -1],
            [-1, -1, -1, -1, 1, -1],
            [-1, -1, 3, -1, -1, -1]]
    assert obs.rows.dtype == np.int8 and obs.rows.tolist() == want
    assert obs.row_offsets.dtype == np.int64 and obs.row_offsets.tolist() == [0, -3, -3, -3, -7]
    assert obs.row_events.dtype == np.int64 and obs.row_events.tolist() == [1, 2, 0, 1, 1]
    assert obs.n == 6
    again = timed_observations(6, np.asarray(nodes), torch.tensor(offsets), [float(k) for k in kinds])
    assert again.rows.tolist() == want and again.row_offsets.tolist() == [0, -3, -3, -3, -7]
    # a node seen twice at one offset: two rows, in input order; no record at offset 0 at all
    twice = timed_observations(3, [2, 2, 0], [-1, -1, -1], [0, 3, 1])
    assert twice.rows.tolist() == [[1, -1, 0], [-1, -1, 3]] and twice.row_offsets.tolist() == [-1, -1] and twice.row_events.tolist() == [1, 1]
    one = timed_observations(2, [1], [0], [0])
    assert one.rows.tolist() == [[-1, 0]] and one.row_offsets.tolist() == [0] and one.row_events.tolist() == [0]


def test_timed_observations_refuses():
    from gnode.dmp import timed_observations
    good = dict(n=6, nodes=[4, 1, 2], offsets=[-3, 0, -1], kinds=[3, 0, 4])
    timed_observations(**good)
    for change in (dict(offsets=[-3, 1, -1]), dict(nodes=[4, 6, 2]), dict(nodes=[4, -1, 2]), dict(kinds=[3, 5, 4]), dict(kinds=[3, -1, 4]),
                   dict(nodes=[4, 1]), dict(offsets=[-3, 0, -1, 0]), dict(kinds=[3, 0]), dict(nodes=[], offsets=[], kinds=[]),
                   dict(kinds=[3, 0.5, 4]), dict(offsets=[-3, float("nan"), -1]), dict(nodes=[[4, 1, 2]]), dict(n=0), dict(n=2.5),
                   dict(n="six")):
        with pytest.raises(ValueError):
            timed_observations(**dict(good, **change))


def test_observations_from_events_on_a_hand_written_trajectory():
    from gnode.dmp import observations_from_events, timed_observations
    #        node: 0   1   2   3   4   5
    t_inf = [0, 2, -1, 7, 3, 5]                                     # 2 is never infected, 3 is infected after now = 5
    t_rec = [1, 6, -1, -1, 5, -1]                                   # 0 and 4 have recovered by now, 1 recovers after it
    sensors = [2, 3, 4, 0, 1]
    assert observations_from_events(t_inf, t_rec, 5, sensors) == ([2, 3, 4, 0, 1], [0, 0, -2, -5, -3], [0, 0, 3, 3, 3])
    assert observations_from_events(t_inf, t_rec, 5, sensors, what="removal") == ([4, 0], [0, -4], [4, 4])
    assert observations_from_events(t_inf, t_rec, 5, sensors, what=("state",)) == ([2, 3, 4, 0, 1], [0] * 5, [0, 0, 2, 2, 1])
    both = observations_from_events(np.asarray(t_inf, dtype=np.int16), torch.tensor(t_rec, dtype=torch.int16), 5, torch.tensor(sensors),
                                    what=("removal", "onset"))
    assert both == ([4, 0, 2, 3, 4, 0, 1], [0, -4, 0, 0, -2, -5, -3], [4, 4, 0, 0, 3, 3, 3])
    obs = timed_observations(6, *both)                              # node 4 at two offsets, node 0 at two others
    assert obs.row_offsets.tolist() == [0, -2, -3, -4, -5] and obs.row_events.tolist() == [1, 1, 1, 1, 1]
    assert obs.rows[0].tolist() == [-1, -1, 0, 0, 4, -1]
    assert observations_from_events(t_inf, t_rec, 0, [0, 1]) == ([0, 1], [0, 0], [3, 0])       # the seed's onset is now
    for bad in (dict(now=-1), dict(sensors=[6]), dict(sensors=[-1]), dict(what=()), dict(what=("onsets",)), dict(t_rec=t_rec[:-1]),
                dict(t_inf=[t_inf], t_rec=[t_rec]), dict(now=2.5)):
        with pytest.raises(ValueError):
            observations_from_events(**dict(dict(t_inf=t_inf, t_rec=t_rec, now=5, sensors=sensors), **bad))


def test_shift_and_add_is_the_explicit_adds_in_ascending_row_order():
    from gnode.dmp import sum_timed_rows
    R, C, T, floor = 5, 3, 6, 1e-6
    table = -np.exp(np.random.default_rng(7).uniform(-3.0, 5.0, size=(R, C, T)))        # log-likelihoods of every size, all < 0
    offsets, events = [0, -2, -2, -5, -9], [2, 1, 0, 3, 1]          # -9: the whole row lies before the outbreak
    before = math.log(float(np.float32(floor)))
    want = np.zeros((C, T))
    for r in range(R):
        term = np.empty((C, T))
        for t in range(T):
            term[:, t] = table[r, :, t + offsets[r]] if t + offsets[r] >= 0 else events[r] * before
        want = want + term
    for given in (table, torch.from_numpy(table)):
        got = sum_timed_rows(given, offsets, events, floor)
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float64 and got.shape == (C, T)
        assert np.array_equal(got.numpy(), want)
    assert got[0, 0].item() == table[0, 0, 0] + before + 0.0 + 3 * before + before       # t = 0: only row 0 has begun
    assert got[1, 5].item() == (((table[0, 1, 5] + table[1, 1, 3]) + table[2, 1, 3]) + table[3, 1, 0]) + before
    none = sum_timed_rows(table[2:3], [-2], [0], floor)             # a row without events costs exactly nothing before the outbreak
    assert none[:, :2].eq(0.0).all() and not torch.signbit(none[:, :2]).any() and np.array_equal(none[:, 2:].numpy(), table[2, :, :4])
    for bad in ((table[0], [0], [1]), (table, offsets[:-1], events), (table, offsets, events[:-1]), (table, [0, 1, 0, 0, 0], events),
                (torch.from_numpy(table).float(), offsets, events)):
        with pytest.raises(ValueError):
            sum_timed_rows(*bad, floor)
