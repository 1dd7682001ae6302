"""No GPU: the Monte-Carlo candidate sweep -- the two entries' binding against the header, the size query and the entry without
a handle, every ValueError of gnode.ode_nn.outbreak_sizes_mc with the library out of reach, and the model
(tests/sir_sweep_model.py): its shift rule, the liveness of every case tests/test_gpu_sir_sweep.py runs, and the tree
comparison's bound on the model alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import schedule_cases as K
import sir_sweep_model as S
from sir_host_cases import N, RING, Reached, lib, no_library  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"gnode_sir_sweep_workspace_bytes": 5, "gnode_sir_mc_philox_sweep": 21}


# --------------------------------------------------------------------------------------------------------------- the ABI
def test_the_two_entries_are_bound_with_the_headers_arity():
    from gnode import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gnode.h")).read(), flags=re.S)
    protos = {name: params for _, name, params in re.findall(r"^(size_t|int)\s*(gnode_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src, flags=re.M)}
    for name, arity in ARITY.items():
        assert name in _lib.EXPORTS and protos[name].count(",") + 1 == arity == len(_lib.ABI[name][1]), name
    assert len(_lib.ABI["gnode_sir_mc_philox_schedule"][1]) == 19   # the scheduled entry is what it was


def test_the_size_query_answers_0_and_the_entry_refuses_without_a_handle(lib):
    assert lib.gnode_sir_sweep_workspace_bytes(None, 10, 2, 12, 5) == 0
    init = np.ascontiguousarray(np.tile([1.0, 0.0, 0.0], (4, 1)))
    cand, phase = np.zeros(1, np.int32), np.zeros(3, np.int32)
    w, gam = np.zeros((1, 6)), np.zeros((1, 4))
    hp = lambda a: a.ctypes.data_as(C.c_void_p)                     # noqa: E731
    status = lib.gnode_sir_mc_philox_sweep(None, hp(init), hp(cand), None, 1, 0, hp(phase), 1, 3, hp(w), hp(gam), 4, 0, 3, C.c_uint64(1),
                                           None, None, None, 0, None, 0)
    assert status == -1 and "gnode_sir_mc_philox_sweep" in lib.gnode_last_error().decode()


# --------------------------------------------------------------------------------------------------------------- refusals
def test_outbreak_sizes_mc_refuses_before_the_library(no_library):
    import torch
    from gnode.ode_nn import InitialState, edge_rates, outbreak_sizes_mc, rate_schedule
    short = rate_schedule([0.2, 0.4], steps=[0, 0, 0, 1, 1, 0])     # names 6 entries: calendar steps up to 5
    good = dict(graph=RING, beta=0.3, gamma=0.2, sims=10, maxTime=4, candidates=[0, 3, -1], start=[1])
    bad = [
        dict(shifts=[0, -1, 2]), dict(shifts=[0, 1.5, 2]), dict(shifts=[0, 1]), dict(shifts=[0, 1, 2, 3]), dict(shifts=3), dict(shifts="now"),
        dict(gamma=short, shifts=[0, 3, 0]), dict(gamma=short, maxTime=7), dict(beta=short, shifts=[0, 0, 9]),   # steps= shorter than max shift + maxTime
        dict(beta=1.5), dict(beta=float("nan")), dict(gamma=-0.1), dict(beta=[0.3] * (N - 1)), dict(gamma=rate_schedule([0.2, 1.5], starts=[1, 3])),
        dict(beta=edge_rates(RING, np.full(2 * N, 0.3)), graph=(np.arange(0, 2 * N - 1, 2), RING[1][:2 * N - 2] % (N - 1))),   # rates of another graph
        dict(gamma=edge_rates(RING, np.full(2 * N, 0.3))),
        dict(candidates=[0, N]), dict(candidates=[-2]), dict(candidates=[]), dict(candidates=[0.5]),
        dict(action="cure"), dict(action="immunise", start=None), dict(action="immunise", start=InitialState.from_sets(N, [], [2])),
        dict(start=[N]), dict(start=InitialState.from_sets(N + 1, [1])),
        dict(maxTime=0), dict(maxTime=2.5), dict(sims=-1), dict(sims=2.5), dict(sim_offset=-1), dict(sims=10, sim_offset=2**32),
        dict(sums=torch.zeros((3, 4, 3), dtype=torch.int32)), dict(sums=torch.zeros((2, 4, 3), dtype=torch.int64)), dict(sums=np.zeros((3, 4, 3))),
    ]
    for change in bad:
        with pytest.raises(ValueError):
            outbreak_sizes_mc(**dict(good, **change))
    for ok in (good, dict(good, shifts=[0, 2, 5]), dict(good, gamma=short, shifts=[0, 2, 0]), dict(good, action="immunise"),
               dict(good, candidates=None), dict(good, start=None), dict(good, maxTime=1), dict(good, sims=0),
               dict(good, beta=rate_schedule([0.3, edge_rates(RING, np.full(2 * N, 0.1))], starts=[1, 3]), gamma=np.full(N, 0.2)),
               dict(good, sums=torch.zeros((3, 4, 3), dtype=torch.int64))):
        with pytest.raises(Reached):                                # everything was in order: the next thing is the library
            outbreak_sizes_mc(**ok)


# --------------------------------------------------------------------------------------------------------------- the model
def test_a_shift_moves_the_phase_row_and_an_id_outside_the_graph_changes_nothing():
    from sir_schedule_model import schedule_thresholds, sir_events_schedule
    import sir_model as M
    n, rp, ci, W, G, p = K.tree()
    phase, T, sims = K.TREE_PHASE, 6, 50
    cands, shifts = [3, 3, 40, -1, n], [0, 4, 6, 2, 2]
    for action in ("seed", "immunise"):
        sums, ever = S.sweep(n, rp, ci, p, cands, shifts, action, W, G, phase, sims, T, 9, sim_offset=5)
        assert sums.shape == (5, T, 3) and ever.shape == (5, sims) and (sums.sum(2) == sims * n).all()
        for j, (c, k) in enumerate(zip(cands, shifts)):             # (c, shift k) under a row = (c, shift 0) under the row moved by k
            a, b = S.sweep(n, rp, ci, p, [c], [0], action, W, G, phase[k:], sims, T, 9, sim_offset=5)
            assert np.array_equal(a[0], sums[j]) and np.array_equal(b[0], ever[j])
        assert np.array_equal(sums[0, 0], sums[1, 0]) and not np.array_equal(sums[0], sums[1])       # one start, two shifts
        assert np.array_equal(sums[3], sums[4]) and np.array_equal(ever[3], ever[4])                 # -1 and n: the start as it is
        assert np.array_equal(S.infections(sums), ever.sum(1, dtype=np.int64))
    THR, TG = schedule_thresholds(W, G, len(ci), n)                 # "no change" is the scheduled call's own curves, summed
    t_inf, t_rec = sir_events_schedule(n, rp, ci, p, THR, TG, phase[2:], sims, T, 9, 5)
    assert np.array_equal(sums[3], M.curves(t_inf, t_rec, T).sum(0))
    v = int(np.flatnonzero(p[:, 0] == 1.0)[0])                      # a node that starts susceptible in every trajectory
    row0 = lambda action: S.sweep(n, rp, ci, p, [-1, v], [0, 0], action, W, G, phase, sims, T, 9)[0][:, 0].astype(np.int64)     # noqa: E731
    assert np.array_equal(np.diff(row0("immunise"), axis=0)[0], [-sims, 0, sims])       # row 0 is the start after the override
    assert np.array_equal(np.diff(row0("seed"), axis=0)[0], [-sims, sims, 0])


@pytest.mark.parametrize("key,action,shifts", S.RUNS)
def test_every_case_of_the_gpu_module_is_live(key, action, shifts):
    S.live(key, action, shifts)


def test_the_tree_comparison_holds_for_the_model_alone():
    """Every eighth node of the tree (all 120 were checked once, see tests/test_gpu_sir_sweep.py): DMP's expected number ever
    infected against the model's trajectories, inside 5 std / sqrt(sims) + 1 / sims."""
    cands = list(range(0, 120, 8))
    ratio = S.tree_ratio(S.tree_dmp(cands), S.tree_ever(cands))
    print("largest share of the bound:", float(ratio.max()))
    assert ratio.max() <= 1.0
