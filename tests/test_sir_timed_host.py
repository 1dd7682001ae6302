"""No GPU: the Monte-Carlo source scores from timed evidence -- the two entries' binding against the header, the size query and
the entry without a handle, every ValueError of gnode.ode_nn.source_scores_timed_mc with the library out of reach, and the
model's restatement of gnode.dmp's record rule and packing held against gnode.dmp itself."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sir_timed_model as TM
from sir_host_cases import N, RING, Reached, _obs, lib, no_library, shared_refusals  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"gnode_sir_sweep_timed_workspace_bytes": 7, "gnode_sir_mc_philox_sweep_timed": 27}


# --------------------------------------------------------------------------------------------------------------- the ABI
def test_the_two_entries_are_bound_with_the_headers_arity():
    from gnode import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gnode.h")).read(), flags=re.S)
    protos = {name: params for _, name, params in re.findall(r"^(size_t|int)\s*(gnode_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src, flags=re.M)}
    for name, arity in ARITY.items():
        assert name in _lib.EXPORTS and protos[name].count(",") + 1 == arity == len(_lib.ABI[name][1]), name
    assert len(_lib.ABI["gnode_sir_mc_philox_sweep"][1]) == 21 and len(_lib.ABI["gnode_sir_mc_philox_sweep_scores"][1]) == 24   # what they were
    # the scores' arguments with the snapshot's (obs, O, measure, bins) replaced by (four record arrays, R, O, bins)
    scores, timed = _lib.ABI["gnode_sir_mc_philox_sweep_scores"][1], _lib.ABI["gnode_sir_mc_philox_sweep_timed"][1]
    assert timed[:11] == scores[:11] and timed[18:] == scores[15:] and timed[11:18] == [C.c_void_p] * 4 + [C.c_int32] * 3


def test_the_version_stays_and_the_entry_refuses_without_a_handle(lib):
    assert lib.gnode_version() == 226                               # a stale library is known by the missing symbol
    assert lib.gnode_sir_sweep_timed_workspace_bytes(None, 10, 2, 12, 5, 3, 9) == 0
    init = np.ascontiguousarray(np.tile([1.0, 0.0, 0.0], (4, 1)))
    cand, phase, rec = np.zeros(1, np.int32), np.zeros(3, np.int32), np.zeros(1, np.int32)
    w, gam = np.zeros((1, 6)), np.zeros((1, 4))
    hp = lambda a: a.ctypes.data_as(C.c_void_p)                     # noqa: E731
    status = lib.gnode_sir_mc_philox_sweep_timed(None, hp(init), hp(cand), None, 1, 0, hp(phase), 1, 3, hp(w), hp(gam), hp(rec), hp(rec), hp(rec), hp(rec),
                                                 1, 1, 1, 4, 0, 3, C.c_uint64(1), None, None, 0, None, 0)
    assert status == -1 and "gnode_sir_mc_philox_sweep_timed" in lib.gnode_last_error().decode()


# --------------------------------------------------------------------------------------------------------------- refusals
def test_source_scores_timed_mc_refuses_before_the_library(no_library):
    import torch
    from gnode.dmp import timed_observations
    from gnode.ode_nn import rate_schedule, source_scores_timed_mc
    short = rate_schedule([0.2, 0.4], steps=[0, 0, 0, 1, 1, 0])     # names 6 entries: calendar steps up to 5
    ev = timed_observations(N, [0, 2, 2, 5], [0, -1, 0, -3], [1, 3, 2, 0])
    row = [0, 1, 4, -1, 3, 0]
    good = dict(graph=RING, observations=ev, beta=0.3, gamma=0.2, sims=10, maxTime=4, candidates=[0, 3, -1])
    many = _obs(np.zeros((1000, N), np.int8), -np.arange(1000))      # 6 000 records
    bad = [
        dict(observations=None), dict(observations=[]), dict(observations=np.asarray(row, np.int8)), dict(observations=[ev, row]), dict(observations=7),
        dict(observations=_obs([row[:5]], [0], n=5)), dict(observations=_obs([row], [0], n=5)), dict(observations=_obs(row, [0])),
        dict(observations=_obs([row], [0, -1])), dict(observations=_obs([row], [1])), dict(observations=_obs([row], [0.0])),
        dict(observations=_obs(np.asarray([row], float), [0])), dict(observations=_obs([[0, 1, 5, -1, 3, 0]], [0])),
        dict(observations=_obs([[0, 1, -2, -1, 3, 0]], [0])), dict(observations=_obs([[-1] * N], [0])), dict(observations=[ev, _obs([[-1] * N], [0])]),
        dict(observations=_obs(np.zeros((0, N), np.int8), np.zeros(0, np.int64))),
        dict(observations=many),                                    # the default bins would be 6 000: asks for bins
        dict(bins=0), dict(bins=4097), dict(bins=2.5), dict(bins="many"),
        dict(maxTime=2049), dict(bins=4096, candidates=list(range(N)) * 5000, maxTime=20),    # 30 000 x 20 x 4097 cells >= 2^31
        dict(hist=torch.zeros((1, 3, 4, 5), dtype=torch.int32)), dict(hist=torch.zeros((3, 4, 5), dtype=torch.int64)), dict(hist=np.zeros((1, 3, 4, 5))),
        dict(hist=torch.zeros((1, 3, 4, 4), dtype=torch.int64)), dict(observations=[ev, ev], hist=torch.zeros((1, 3, 4, 5), dtype=torch.int64)),
        *shared_refusals(),                                         # what outbreak_sizes_mc refuses, through the shared checks
    ]
    for change in bad:
        with pytest.raises(ValueError):
            source_scores_timed_mc(**dict(good, **change))
    with pytest.raises(ValueError, match="give bins"):
        source_scores_timed_mc(**dict(good, observations=many))
    with pytest.raises(TypeError):
        source_scores_timed_mc(**dict(good, action="immunise"))     # the action is fixed: a source is seeded
    with pytest.raises(TypeError):
        source_scores_timed_mc(**dict(good, measure="match"))       # and so is the measure: the records matched
    for ok in (good, dict(good, observations=[ev, ev]), dict(good, observations=[ev] * 17), dict(good, observations=(ev,)),
               dict(good, observations=_obs([row], [0])), dict(good, observations=_obs(torch.tensor([row], dtype=torch.int8), torch.tensor([-2]))),
               dict(good, observations=_obs(np.asarray([row, row], np.int64), [-(2**40), 0])), dict(good, observations=many, bins=64),
               dict(good, bins=7), dict(good, bins=4096), dict(good, maxTime=2048), dict(good, observations=[ev] * 40, maxTime=200),
               dict(good, shifts=[0, 2, 5]), dict(good, gamma=short, shifts=[0, 2, 0]), dict(good, candidates=None), dict(good, start=[1]),
               dict(good, start=None), dict(good, sims=0), dict(good, hist=torch.zeros((1, 3, 4, 5), dtype=torch.int64)),
               dict(good, observations=[ev] * 17, hist=torch.zeros((17, 3, 4, 5), dtype=torch.int64))):
        with pytest.raises(Reached):                                # everything was in order: the next thing is the library
            source_scores_timed_mc(**ok)


# ------------------------------------------------------------------------------------------- the model's restatements
def test_the_models_rule_and_packing_are_gnode_dmps():
    from gnode.dmp import observations_from_events, timed_observations
    from gnode.ode_nn import _timed_records
    rng = np.random.default_rng(2)
    n = 12
    for now in (0, 3, 7):
        t_inf = rng.integers(-1, 9, n)
        t_rec = np.where((t_inf >= 0) & (rng.random(n) < 0.7), t_inf + rng.integers(0, 4, n), -1)
        sensors = [1, 4, 5, 8, 11, 4]
        mine = TM.reports(t_inf, t_rec, now, sensors)
        nodes, offsets, kinds = observations_from_events(t_inf, t_rec, now, sensors, what=("onset", "removal", "state"))
        assert mine == list(zip(nodes, offsets, kinds))
        theirs, packed = timed_observations(n, nodes, offsets, kinds), TM.Observations(n, mine)
        assert np.array_equal(theirs.rows, packed.rows) and np.array_equal(theirs.row_offsets, packed.row_offsets) and theirs.n == packed.n
        # what the library is handed: the records by row, then by node
        squeezed, sets = _timed_records("test", theirs, n)
        assert squeezed and len(sets) == 1 and sorted(zip(*(a.tolist() for a in sets[0]))) == sorted(mine)
        assert list(zip(*(a.tolist() for a in sets[0]))) == TM.records_of(packed)
        assert _timed_records("test", [theirs, packed], n)[0] is False
