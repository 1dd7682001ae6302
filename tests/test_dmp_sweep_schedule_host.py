"""No GPU: source scores and outbreak sizes under a rate schedule -- the four entries' binding against the header, every
ValueError of gnode.dmp.source_scores_schedule and outbreak_sizes_schedule with the library out of reach, and the model
(tests/dmp_sweep_schedule_model.py): its shift, its diagonal, and the sanity case that tests/test_gpu_dmp_sweep_schedule.py
holds the device to."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import dmp_sweep_schedule_model as M
import schedule_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"gnode_dmp_source_events_schedule_workspace_bytes": 5, "gnode_dmp_source_events_scores_schedule_f32": 18,
         "gnode_dmp_outbreak_schedule_workspace_bytes": 4, "gnode_dmp_outbreak_sizes_schedule_f32": 17}


# --------------------------------------------------------------------------------------------------------------- the ABI
def test_the_four_entries_are_bound_with_the_headers_arity():
    from gnode import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gnode.h")).read(), flags=re.S)
    protos = {name: params for _, name, params in re.findall(r"^(size_t|int)\s*(gnode_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src, flags=re.M)}
    for name, arity in ARITY.items():
        assert name in _lib.EXPORTS and protos[name].count(",") + 1 == arity == len(_lib.ABI[name][1]), name
    # the constant entries are what they were
    assert len(_lib.ABI["gnode_dmp_source_events_scores_f32"][1]) == 14 and len(_lib.ABI["gnode_dmp_outbreak_sizes_f32"][1]) == 13


def test_the_units_are_built_and_attributes_are_set_for_the_one_workgroup_instances():
    from gnode import build
    csrc = os.path.join(ROOT, "gn-ode-sir_amd", "csrc")
    for unit in ("gnode_dmp_source_events_schedule.hip", "gnode_dmp_outbreak_schedule.hip"):
        assert unit in build.SOURCES and os.path.exists(os.path.join(csrc, unit))
    create = open(os.path.join(csrc, "gnode_ode.hip")).read()
    for setter in ("gn_dmp_source_events_schedule_set_attributes", "gn_dmp_outbreak_schedule_set_attributes"):
        assert f"{setter}()" in create                             # more than 64 KiB of dynamic LDS needs the attribute


# --------------------------------------------------------------------------------------------------------------- refusals
class Reached(Exception):
    pass


@pytest.fixture
def no_library(monkeypatch):
    from gnode import _lib, dmp

    def refuse(*a, **k):
        raise Reached("the library was loaded, or a DeviceGraph made")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(dmp, "DeviceGraph", refuse)


N = 6


def _ring(w=0.3, n=N):
    rows = np.arange(n)
    return sp.csr_matrix((np.full(2 * n, w), (np.r_[rows, rows], np.r_[(rows + 1) % n, (rows - 1) % n])), shape=(n, n))


def _chain(w=0.3, n=N):                                             # another sparsity pattern on the same nodes
    rows = np.arange(n - 1)
    return sp.csr_matrix((np.full(2 * (n - 1), w), (np.r_[rows, rows + 1], np.r_[rows + 1, rows])), shape=(n, n))


ROWS = [[1, 2, 0, -1, 3, 4]]


def test_source_scores_schedule_refuses_before_the_library(no_library):
    from gnode.dmp import source_scores_schedule
    from gnode.ode_nn import rate_schedule
    lock = rate_schedule([_ring(0.3), _ring(0.1)], starts=[1, 4])
    short = rate_schedule([0.2, 0.4], steps=[0, 0, 0, 1, 1, 0])     # names 6 entries: calendar steps up to 5
    good = dict(weight_adj=lock, rows=ROWS, gamma=0.2, maxTime=4)
    bad = [
        dict(observed_at=2), dict(observed_at=-1), dict(observed_at=3.5), dict(observed_at="soon"),       # < maxTime - 1, or no whole number
        dict(gamma=short, observed_at=6), dict(gamma=short, maxTime=7),                                  # steps= shorter than D + 1, than maxTime
        dict(scale=short, observed_at=9),
        dict(weight_adj=rate_schedule([_ring(), _chain()], starts=[1, 3])),                              # the phases' patterns differ
        dict(scale=rate_schedule([1.0, 4.0], starts=[1, 3])), dict(scale=4.0),                           # a weight times its scale > 1
        dict(gamma=rate_schedule([0.2, 1.5], starts=[1, 3])), dict(gamma=float("nan")), dict(gamma=-0.1),
        dict(scale=rate_schedule([[1.0] * 2, 0.5], starts=[1, 2])),                                      # per-sample scales: the tables are shared
        dict(rows=[[1, 2, 0, -1, 3, 5]]), dict(rows=[[1, 2, 0, -2, 3, 4]]), dict(rows=[[1.5, 2, 0, -1, 3, 4]]),      # codes outside -1 .. 4
        dict(rows=[[1, 2, 0]]), dict(rows=[1, 2, 0, -1, 3, 4]), dict(rows=[]),
        dict(candidates=[0, N]), dict(candidates=[-1]), dict(candidates=[]), dict(candidates=[0.5]),    # a candidate outside the graph
        dict(maxTime=1), dict(maxTime=2.5), dict(floor=0.0), dict(floor=2.0), dict(floor=float("nan")), dict(floor=1e-60),
        dict(budget_bytes=0),
    ]
    for change in bad[:-1]:
        with pytest.raises(ValueError):
            source_scores_schedule(**dict(good, **change))
    for ok in (good, dict(good, observed_at=3), dict(good, gamma=short, observed_at=5), dict(good, gamma=short, maxTime=6),
               dict(good, weight_adj=_ring(), scale=rate_schedule([1.0, 0.25], starts=[1, 3]))):
        with pytest.raises(Reached):                                # everything was in order: the next thing is the library
            source_scores_schedule(**ok)


def test_outbreak_sizes_schedule_refuses_before_the_library(no_library):
    from gnode.dmp import outbreak_sizes_schedule
    from gnode.ode_nn import rate_schedule
    lock = rate_schedule([_ring(0.3), _ring(0.1)], starts=[1, 4])
    short = rate_schedule([0.2, 0.4], steps=[0, 0, 0, 1, 1, 0])
    good = dict(weight_adj=lock, gamma=0.2, maxTime=4, candidates=[0, 3, -1], start=[1])
    bad = [
        dict(shifts=[0, -1, 2]), dict(shifts=[0, 1.5, 2]), dict(shifts=[0, 1]), dict(shifts=[0, 1, 2, 3]), dict(shifts=3),
        dict(shifts=[[0, 1, 2]]), dict(shifts="now"),                                                    # negative, fractional, wrong count
        dict(gamma=short, shifts=[0, 3, 0]), dict(gamma=short, maxTime=7),                               # steps= shorter than max shift + maxTime
        dict(weight_adj=rate_schedule([_ring(), _chain()], starts=[1, 3])),
        dict(scale=rate_schedule([1.0, 4.0], starts=[1, 3])), dict(gamma=rate_schedule([0.2, 1.5], starts=[1, 3])),
        dict(candidates=[0, N]), dict(candidates=[-2]), dict(candidates=[]),
        dict(action="cure"), dict(action="immunise", start=None), dict(start=[N]), dict(value=[1.0] * (N - 1)), dict(value=[-1.0] * N),
        dict(maxTime=1),
    ]
    for change in bad:
        with pytest.raises(ValueError):
            outbreak_sizes_schedule(**dict(good, **change))
    for ok in (good, dict(good, shifts=[0, 2, 5]), dict(good, gamma=short, shifts=[0, 2, 0]), dict(good, action="immunise"),
               dict(good, value=np.arange(N))):
        with pytest.raises(Reached):
            outbreak_sizes_schedule(**ok)


def test_the_constant_calls_name_the_new_ones_when_they_refuse_a_schedule(no_library):
    from gnode import dmp
    from gnode.ode_nn import rate_schedule
    s = rate_schedule([0.2, 0.1], starts=[1, 3])
    for call in (lambda: dmp.source_scores_events(_ring(), ROWS, s, 4), lambda: dmp.outbreak_sizes(_ring(), s, 4)):
        with pytest.raises(ValueError, match="source_scores_schedule, outbreak_sizes_schedule"):
            call()


# --------------------------------------------------------------------------------------------------------------- the model
def test_a_shift_moves_the_phase_row_and_equal_tables_change_nothing():
    from dmp_schedule_model import dmp_sir_schedule
    n, rp, ci, W, G, p = schedule_cases.tree()
    phase, T = schedule_cases.TREE_PHASE, 5
    rows = np.random.default_rng(1).integers(-1, 5, (2, n)).astype(np.int8)
    cands, shifts = [3, 3, 40], [0, 4, 7]
    table = M.scores(rp, ci, W, G, phase, cands, shifts, rows, T)
    assert table.shape == (2, 3, T) and np.isfinite(table).all()
    for j, (c, s) in enumerate(zip(cands, shifts)):                 # (c, shift s) under a row = (c, shift 0) under the row moved by s
        assert np.array_equal(M.scores(rp, ci, W, G, phase[s:], [c], [0], rows, T)[:, 0], table[:, j])
    assert np.array_equal(table[:, 0, 0], table[:, 1, 0]) and not np.array_equal(table[:, 0], table[:, 1])       # one start, two shifts
    same = M.scores(rp, ci, [W[0]] * 3, [G[0]] * 3, phase, cands, shifts, rows, T)
    assert np.array_equal(same, M.scores(rp, ci, W[:1], G[:1], np.zeros(T, dtype=int), cands, [0, 0, 0], rows, T))
    # the sizes are the marginals' column sums: with every node counting 1 a row sums to n
    sz = M.sizes(rp, ci, W, G, phase, p, [-1, 5, 5], [0, 0, 6], "immunise", None, T)
    assert np.allclose(sz.sum(-1), n, rtol=0, atol=1e-3)
    assert np.array_equal(sz[0], dmp_sir_schedule(rp, ci, W, G, phase, p, T).astype(np.float64).sum(1))       # -1: the start as it is
    assert not np.array_equal(sz[1], sz[2])


def test_observed_at_is_the_diagonal_of_one_run_per_start():
    n, rp, ci, W, G, _ = schedule_cases.tree()
    phase, T, D = schedule_cases.TREE_PHASE, 4, 9
    rows = np.random.default_rng(2).integers(-1, 3, (1, n)).astype(np.int8)
    got = M.scores_observed_at(rp, ci, W, G, phase, [7, 50], rows, T, D)
    assert got.shape == (1, 2, T)
    for tau in range(T):                                            # c started tau steps before D: steps D - tau + 1 .. D govern
        row = np.concatenate([[0], phase[D - tau + 1:D + 1], np.zeros(T, dtype=phase.dtype)])[:T]
        assert np.array_equal(M.scores(rp, ci, W, G, row, [7, 50], [0, 0], rows, T)[:, :, tau], got[:, :, tau])


def test_the_sanity_case_finds_the_source_under_the_schedule_and_not_under_constant_rates():
    """The model alone, on the CPU: with observed_at = 13 under the true three-phase calendar the true source 4 is ranked first,
    1.655 ahead of node 5, at tau = 9, the true age of the outbreak; under phase 0's rates held constant node 36 is first, 0.253
    ahead of the true source.  Both gaps are far above 1e-6 relative."""
    s = M.SANITY
    n, rp, ci, W, G, phase, snapshot = M.sanity_case()
    assert len(phase) == s["D"] + 1 and sorted(set(phase[1:].tolist())) == [0, 1, 2] and s["TAU"] < s["T"] <= s["D"] + 1
    assert len(set(phase[s["D"] - s["TAU"] + 1:].tolist())) == 3    # the outbreak meets all three phases
    assert snapshot[0, s["source"]] >= 1 and set(np.unique(snapshot)) == {0, 1, 2}
    cands, scheduled, constant = M.sanity_tables()
    assert np.isfinite(scheduled).all() and np.isfinite(constant).all() and s["source"] in cands and len(cands) >= 5
    order, best = M.ranking(scheduled, cands)
    print(f"scheduled: first {order[0]}, {best[0] - best[1]:.3f} ahead of {order[1]}, at tau = {scheduled[list(cands).index(order[0])].argmax()}")
    assert order[0] == s["source"] and best[0] - best[1] >= 1e-6 * abs(best[0])
    assert scheduled[list(cands).index(s["source"])].argmax() == s["TAU"]
    order_c, best_c = M.ranking(constant, cands)
    at = order_c.index(s["source"])
    print(f"constant: first {order_c[0]}, the true source at rank {at}, {best_c[0] - best_c[at]:.3f} behind")
    assert at > 0 and best_c[0] - best_c[at] >= 1e-6 * abs(best_c[0])
