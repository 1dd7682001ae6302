"""CPU: the host side of rates that change over time -- `rate_schedule` / `RateSchedule.phase_of_step`, the joint phases of
several schedules, the tables the Monte-Carlo and DMP calls build from them, and every ValueError, raised before the library
is entered (`sir_cases.StubGraph`'s handle raises, and `_lib.load` is replaced by a function that does)."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from sir_cases import StubGraph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def no_library(monkeypatch):
    from gnode import _lib

    def load():
        raise AssertionError("the library was entered before the arguments were checked")
    monkeypatch.setattr(_lib, "load", load)


# ------------------------------------------------------------------------------------------------------- rate_schedule
def test_phase_of_step():
    from gnode.ode_nn import rate_schedule
    T = 9
    assert rate_schedule([0.3], starts=[1]).phase_of_step(T).tolist() == [0] * T                      # one value from step 1 on
    assert rate_schedule([0.3, 0.1], starts=[1, T - 1]).phase_of_step(T).tolist() == [0] * (T - 1) + [1]  # a change at T - 1
    assert rate_schedule([0.3, 0.1], starts=[1, 2]).phase_of_step(T).tolist() == [0, 0] + [1] * (T - 2)
    assert rate_schedule([0.3, 0.1, 0.2], starts=[1, 4, 6]).phase_of_step(T).tolist() == [0, 0, 0, 0, 1, 1, 2, 2, 2]
    assert rate_schedule(list(np.linspace(0.1, 0.8, T - 1)), starts=range(1, T)).phase_of_step(T).tolist() == [0] + list(range(T - 1))  # P = T - 1
    assert rate_schedule([0.3, 0.1, 0.2], starts=[1, T, T + 5]).phase_of_step(T).tolist() == [0] * T   # starts at or beyond T are ignored
    week = [0, 0, 0, 0, 0, 1, 1] * 3                                                                  # phases revisited
    s = rate_schedule([0.3, 0.05], steps=[5] + week[1:])                                               # entry 0 is ignored
    assert s.phase_of_step(15).tolist() == [0] + week[1:15] and s.phase_of_step(21).tolist() == [0] + week[1:]
    assert s.phase_of_step(1).tolist() == [0] and s.phase_of_step(15).dtype == np.int32
    assert s.P == 2 and rate_schedule([None, 2.0], starts=[1, 3]).values == [None, 2.0]


def test_rate_schedule_refusals():
    from gnode.ode_nn import rate_schedule
    for kw in (dict(values=[]), dict(values=0.3, starts=[1]), dict(values=[0.3]), dict(values=[0.3], starts=[1], steps=[0, 0]),
               dict(values=[0.3, 0.2], starts=[1]), dict(values=[0.3, 0.2], starts=[0, 3]), dict(values=[0.3, 0.2], starts=[2, 3]),
               dict(values=[0.3, 0.2], starts=[1, 1]), dict(values=[0.3, 0.2, 0.1], starts=[1, 5, 4]), dict(values=[0.3, 0.2], starts=[1, 2.5]),
               dict(values=[0.3, 0.2], starts=[[1, 2]]), dict(values=[0.3, 0.2], starts="ab"), dict(values=[0.3, 0.2], steps=[]),
               dict(values=[0.3, 0.2], steps=[0, 2]), dict(values=[0.3, 0.2], steps=[0, 0, -1]), dict(values=[0.3, 0.2], steps=[0, 0.5]),
               dict(values=[rate_schedule([0.3], starts=[1])], starts=[1])):
        with pytest.raises(ValueError):
            rate_schedule(**kw)
    s = rate_schedule([0.3, 0.2], steps=[0, 1, 0, 1])
    with pytest.raises(ValueError, match="4 steps"):
        s.phase_of_step(5)
    with pytest.raises(ValueError):
        s.phase_of_step(0)


# ------------------------------------------------------------------------------------------------ Monte-Carlo tables
def test_joint_phases_and_tables_of_two_schedules():
    from gnode.ode_nn import _scheduled_rates, edge_rates, joint_phases, rate_schedule
    g, T = StubGraph(), 10
    rng = np.random.default_rng(1)
    b_node, w_edge, g_node = rng.uniform(0, 1, g.n), rng.uniform(0, 1, g.nnz), rng.uniform(0, 1, g.n)
    beta = rate_schedule([0.3, b_node, edge_rates(g, w_edge)], starts=[1, 4, 7])       # scalars, per-node arrays and EdgeRates, mixed
    gamma = rate_schedule([0.2, g_node], steps=[0, 0, 1, 1, 0, 0, 1, 1, 0, 0])         # other change points
    s = _scheduled_rates(beta, gamma, g, T)
    pairs = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 1), (2, 0)]                           # distinct pairs in order of first use
    assert s.phase.tolist() == [0, 0, 1, 1, 2, 2, 3, 4, 5, 5] and s.P == 6 and s.phase.dtype == np.int32
    B = [np.full(g.nnz, 0.3), b_node[g.col], w_edge]                                   # restated: w[q] = beta[col[q]]
    Gm = [np.full(g.n, 0.2), g_node]
    assert s.W.shape == (6, g.nnz) and s.G.shape == (6, g.n) and s.W.dtype == s.G.dtype == np.float64
    for j, (pb, pg) in enumerate(pairs):
        assert np.array_equal(s.W[j], B[pb]) and np.array_equal(s.G[j], Gm[pg])
    assert s.W.flags.c_contiguous and s.G.flags.c_contiguous
    # one schedule next to a constant; T = 1 has no step and one phase
    s = _scheduled_rates(0.4, rate_schedule([0.1, 0.9], starts=[1, 3]), g, 5)
    assert s.phase.tolist() == [0, 0, 0, 1, 1] and np.array_equal(s.W, np.full((2, g.nnz), 0.4)) and s.G[:, 0].tolist() == [0.1, 0.9]
    s = _scheduled_rates(beta, gamma, g, 1)
    assert s.phase.tolist() == [0] and s.P == 1
    assert joint_phases([[0, 1, 1, 0], [0, 0, 1, 0], [5, 2, 2, 2]])[0].tolist() == [0, 0, 1, 2]
    assert joint_phases([[0, 1, 1, 0], [0, 0, 1, 0], [5, 2, 2, 2]])[1] == [(1, 0, 2), (1, 1, 2), (0, 0, 2)]


def test_monte_carlo_refusals_come_before_the_library():
    import networkx as nx
    from gnode.ode_nn import edge_rates, initial_state, rate_schedule, sir_counts, sir_torch, sir_trajectories
    g = StubGraph()
    ok = rate_schedule([0.3, 0.1], starts=[1, 3])
    other = edge_rates((np.asarray([0, 1, 2]), np.asarray([1, 0])), np.asarray([0.5, 0.5]))
    nan_nodes = np.full(g.n, 0.5); nan_nodes[3] = np.nan
    bad = [dict(beta=rate_schedule([0.3, 1.5], starts=[1, 3]), gamma=0.2), dict(beta=rate_schedule([0.3, -0.1], starts=[1, 3]), gamma=0.2),
           dict(beta=rate_schedule([0.3, float("nan")], starts=[1, 3]), gamma=0.2), dict(beta=rate_schedule([0.3, nan_nodes], starts=[1, 3]), gamma=0.2),
           dict(beta=rate_schedule([0.3, np.full(g.n + 1, 0.5)], starts=[1, 3]), gamma=0.2), dict(beta=rate_schedule([0.3, other], starts=[1, 3]), gamma=0.2),
           dict(beta=0.3, gamma=rate_schedule([0.2, 1.01], starts=[1, 3])), dict(beta=0.3, gamma=rate_schedule([0.2, nan_nodes], starts=[1, 3])),
           dict(beta=0.3, gamma=rate_schedule([0.2, edge_rates(g, np.full(g.nnz, 0.5))], starts=[1, 3])),
           dict(beta=ok, gamma=1.5), dict(beta=1.5, gamma=ok), dict(beta=ok, gamma=np.full(g.n - 1, 0.2)),
           dict(beta=rate_schedule([0.3, 0.1], steps=[0, 0, 1, 1]), gamma=0.2)]       # fewer steps than the call's T
    for kw in bad:
        with pytest.raises(ValueError):
            sir_counts(g, [0], sims=4, T=6, rng_seed=1, device="cpu", **kw)
        with pytest.raises(ValueError):
            sir_trajectories(g, [0], sims=4, T=6, rng_seed=1, device="cpu", **kw)
        with pytest.raises(ValueError):
            sir_counts(g, initial_state(np.tile([0.5, 0.5, 0.0], (g.n, 1))), sims=4, T=6, rng_seed=1, device="cpu", **kw)
    with pytest.raises(ValueError):
        sir_counts(g, initial_state(np.tile([0.5, 0.5, 0.0], (g.n + 1, 1))), ok, 0.2, 4, 6, 1, device="cpu")
    with pytest.raises(ValueError, match="events hold int16"):
        sir_trajectories(g, [0], ok, 0.2, sims=4, T=40000, rng_seed=1, device="cpu")
    G = nx.path_graph(5)
    for kw in (dict(beta=ok, gamma=0.2), dict(beta=0.3, gamma=ok)):
        with pytest.raises(ValueError, match="RateSchedule"):
            sir_torch(G, [0], sims=2, T=4, coins=np.zeros(100), **kw)


# ------------------------------------------------------------------------------------------------------------- dmp_batch
def _ring(n=6, w=0.3):
    rows = np.arange(n)
    return sp.csr_matrix((np.full(2 * n, w), (np.r_[rows, rows], np.r_[(rows + 1) % n, (rows - 1) % n])), shape=(n, n))


def test_dmp_batch_refusals_come_before_the_library(no_library):
    from gnode.dmp import dmp_batch
    from gnode.ode_nn import rate_schedule
    M, n, B = _ring(), 6, 2
    starts = [[0], [3]]
    sch = lambda v: rate_schedule(v, starts=[1, 3])      # noqa: E731
    missing = M.tolil(); missing[0, 1] = 0; missing = missing.tocsr(); missing.eliminate_zeros()
    bad = [dict(weight_adj=M, gamma=sch([0.2, -0.1])), dict(weight_adj=M, gamma=sch([0.2, float("nan")])),
           dict(weight_adj=M, gamma=sch([0.2, np.full(n + 1, 0.1)])), dict(weight_adj=M, gamma=sch([0.2, np.full((B + 1, n), 0.1)])),
           dict(weight_adj=M, gamma=0.2, scale=sch([None, -1.0])), dict(weight_adj=M, gamma=0.2, scale=sch([None, [1.0, 2.0, 3.0]])),
           dict(weight_adj=M, gamma=0.2, scale=sch([1.0, float("inf")])), dict(weight_adj=M, gamma=0.2, scale=sch([1.0, "x"])),
           dict(weight_adj=M, gamma=0.2, scale=sch([None, 5.0])), dict(weight_adj=M, gamma=sch([0.2, 1.5])),      # probabilities: at most 1
           dict(weight_adj=sch([M, _ring(6, 1.25)]), gamma=0.2),
           dict(weight_adj=sch([M, missing]), gamma=0.2), dict(weight_adj=sch([M, _ring(7)]), gamma=0.2),
           dict(weight_adj=M, gamma=rate_schedule([0.2, 0.1], steps=[0, 0, 1]))]      # fewer steps than maxTime
    for kw in bad:
        with pytest.raises(ValueError):
            dmp_batch(starts=starts, maxTime=5, **kw)
    with pytest.raises(ValueError):
        dmp_batch(M, starts, sch([0.2, 0.1]), 1)
    with pytest.raises(ValueError):
        dmp_batch(M, [], sch([0.2, 0.1]), 5)
    with pytest.raises(ValueError):
        dmp_batch(M, [[0], [n]], sch([0.2, 0.1]), 5)


def test_calls_outside_the_scope_refuse_a_schedule(no_library):
    import torch
    from gnode import dmp, ode_nn
    s = ode_nn.rate_schedule([0.2, 0.1], starts=[1, 3])
    M, n = _ring(), 6
    g = StubGraph()
    for call in (lambda: dmp.DMP_SIR(M, s), lambda: dmp.DMP_SIR(s, [0.2] * n), lambda: dmp.DmpGraph(s),
                 lambda: dmp.dmp_marginals(dmp.DmpGraph(M), s, torch.zeros(n), torch.zeros(1, n, 3), 4),
                 lambda: dmp.dmp_marginals(dmp.DmpGraph(M), torch.zeros(2 * n), s, torch.zeros(1, n, 3), 4),
                 lambda: dmp.source_scores(M, [1] + [-1] * (n - 1), s, 4), lambda: dmp.source_scores(s, [1] + [-1] * (n - 1), 0.2, 4),
                 lambda: dmp.source_scores_batch(M, [[1] + [-1] * (n - 1)], s, 4), lambda: dmp.source_scores_events(M, [[3] + [-1] * (n - 1)], s, 4),
                 lambda: dmp.outbreak_sizes(M, s, 4), lambda: dmp.outbreak_sizes(s, 0.2, 4),
                 lambda: dmp.greedy_seeds(M, s, 4, 1), lambda: dmp.greedy_immunisation(M, [0], s, 4, 1),
                 lambda: ode_nn.runge_kutta_order4(ode_nn.sir, M, n, [0], s, 0.2), lambda: ode_nn.runge_kutta_order4(ode_nn.sir, M, n, [0], 0.3, s),
                 lambda: ode_nn.meanfield_batch(g, [[0]], s, 0.2), lambda: ode_nn.meanfield_batch(g, [[0]], 0.3, s),
                 lambda: ode_nn.meanfield_marginals(g, torch.zeros(1, g.n, 3, dtype=torch.float64), s, torch.zeros(g.n, dtype=torch.float64))):
        with pytest.raises(ValueError):
            call()


# --------------------------------------------------------------------------------------------------------------- the ABI
def test_the_new_entries_are_bound_with_the_headers_arity():
    from gnode import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gnode.h")).read(), flags=re.S)
    protos = {name: params for _, name, params in re.findall(r"^(size_t|int)\s*(gnode_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src, flags=re.M)}
    for name, arity in (("gnode_sir_schedule_workspace_bytes", 3), ("gnode_sir_mc_philox_schedule", 19),
                        ("gnode_dmp_batch_schedule_workspace_bytes", 3), ("gnode_dmp_batch_schedule_f32", 14)):
        assert name in _lib.EXPORTS and protos[name].count(",") + 1 == arity == len(_lib.ABI[name][1]), name
